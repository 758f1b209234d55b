"""The training-step checker (tests/train_oracle.py) catches what it is for -- CPU oracle only, no kernel involved.

On grid case c (B=5, L=50, lengths [50, 31, 44, 50, 38]) a wrong set of gradients is built from the oracle's own fp32 gradients, one
class of kernel bug at a time, and `compare` must report each; the oracle's fp32 gradients themselves must pass.  The lines that are
wrong on purpose live only here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import train_oracle as T  # noqa: E402


@pytest.fixture(scope="module")
def case_c(seeded_sd):
    batch, noise, margins = T.case_inputs(seeded_sd, "c")
    g64, g32, l32 = T.oracle_truth(seeded_sd, batch, noise)
    return batch, noise, margins, g64, g32, l32


def _names(report):
    return {n for n, _, _ in report["bad"]}


def test_ragged_lengths_of_the_grid_are_the_seeded_ones():
    for case, (lo, seed) in T.RAGGED.items():
        B, L, lengths = T.GRID[case][:3]
        assert lengths == T.ragged(B, L, lo, seed), case
    for case, (B, L, lengths, n_gen, _) in T.GRID.items():
        assert len(lengths) == B and lengths[0] == L and max(lengths) == L and min(lengths) > n_gen, case
    assert T.D_REPLAY[:2] == T.GRID["d"][:2] and T.D_REPLAY[2] != T.GRID["d"][2]


def test_condition_leaves_the_asserted_margins_and_is_idempotent(seeded_sd, case_c):
    batch, noise, margins = case_c[:3]
    T.assert_margins(margins)
    assert margins["draw_gap"] >= 0.05 and margins["angle_switch"] >= 1e-3 and margins["torus_wrap"] >= 1e-4
    assert margins["n_generated"] == 5 * 16
    before = {k: v.clone() for k, v in noise.items()}
    again = T.condition(seeded_sd, batch, noise, seed=T.GRID["c"][4])
    assert margins["head_gate"] >= 1.0
    assert again["rounds"] == 0 and again["widened"] == again["rot_redrawn"] == again["ang_redrawn"] == again["gate_redrawn"] == 0
    for k, v in noise.items():
        assert torch.equal(v, before[k]), k
    for k in ("draw_gap", "angle_switch", "torus_wrap", "head_gate", "n_pi_branch"):
        assert again[k] == margins[k], k


def test_condition_moves_a_residue_off_a_switch(seeded_sd):
    """A generated residue put ON the pi switch of so3_log (rot0 = R1 rotated by the switch angle) and a torus difference put on
    the wrap are re-drawn; context residues and the rest of the noise are left alone."""
    import math
    from oracle import pepflow_oracle as O
    B, L, lengths, n_gen, seed = T.GRID["a"]
    batch, noise = T.make_case(B, L, lengths, n_gen, seed)
    T.condition(seeded_sd, batch, noise, seed=seed)
    gen = batch["generate_mask"]
    b, i = [int(v) for v in gen.nonzero()[0]]
    R1 = O.encode(seeded_sd, batch)[0]
    w = torch.tensor([0.0, 0.0, T.SWITCH_PI + 2e-4])
    noise["rot0"][b, i] = R1[b, i] @ O.so3_exp(w[None])[0].T                # rot0^T R1 = exp(w): theta 2e-4 from the switch
    noise["ang0"][b, i, 0] = (batch["torsion_angle"][b, i, 0] + math.pi - 2e-5) % (2 * math.pi)
    before = {k: v.clone() for k, v in noise.items()}
    with torch.no_grad():
        sd64, b64 = T._to64(seeded_sd), T._to64(batch)
        p = T._probe(seeded_sd, batch, O.encode(seeded_sd, batch), noise, sd64, b64, O.encode(sd64, b64))
    assert p["switch"][b, i] < T.ANGLE_MARGIN and p["wrap"][b, i, 0] < T.WRAP_MARGIN
    m = T.condition(seeded_sd, batch, noise, seed=seed)
    assert m["rot_redrawn"] >= 1 and m["ang_redrawn"] >= 1 and m["rounds"] >= 1
    assert not torch.equal(noise["rot0"][b, i], before["rot0"][b, i]) and noise["ang0"][b, i, 0] != before["ang0"][b, i, 0]
    for k in ("rot0", "ang0", "expo"):
        v, w0 = (noise[k], before[k]) if k != "expo" else (noise[k].permute(1, 2, 0, 3), before[k].permute(1, 2, 0, 3))
        assert torch.equal(v[~gen], w0[~gen]), k
    for k in ("t", "trans0", "simplex0"):
        assert torch.equal(noise[k], before[k]), k


def test_condition_moves_a_residue_off_a_head_gate(seeded_sd):
    """A bias of angle_net.0 shifted so that ONE pre-activation of one generated residue is 1e-8 in float64 (below what an fp32
    forward resolves): the residue is flagged, re-drawn, and the asserted head_gate margin holds afterwards."""
    from oracle import pepflow_oracle as O
    B, L, lengths, n_gen, seed = T.GRID["a"]
    batch, noise = T.make_case(B, L, lengths, n_gen, seed)
    T.condition(seeded_sd, batch, noise, seed=seed)
    gen = batch["generate_mask"]
    b, i = [int(v) for v in gen.nonzero()[3]]
    unit, key = 23, "ga_encoder.angle_net.0.bias"
    with torch.no_grad():
        sd64, b64 = T._to64(seeded_sd), T._to64(batch)
        enc64 = O.encode(sd64, b64)
        col = {}
        O.ga_encoder(sd64, *O.corrupt(b64, enc64, T._to64(noise)), enc64[4], enc64[5], batch["res_mask"].long(), collect=col)
        pre = T._head_preactivations(sd64, col[f"s_{O.N_BLOCKS - 1}"])[b, i, 2, unit]          # [B,L,(seq 0, seq 2, angle 0, angle 2),128]
    sd = dict(seeded_sd)
    sd[key] = seeded_sd[key].clone()
    sd[key][unit] = (seeded_sd[key][unit].double() - pre + 1e-8).float()
    with torch.no_grad():
        sd64 = T._to64(sd)
        p = T._probe(sd, batch, O.encode(sd, batch), noise, sd64, b64, O.encode(sd64, b64))
    assert p["gate"][b, i] < 1e-2 * T.GATE_MARGIN, p["gate"][gen]
    before = noise["rot0"].clone()
    m = T.condition(sd, batch, noise, seed=seed)
    assert m["gate_redrawn"] >= 1 and m["head_gate"] >= T.GATE_MARGIN
    assert not torch.equal(noise["rot0"][b, i], before[b, i]) and torch.equal(noise["rot0"][~gen], before[~gen])


def test_compare_passes_the_oracles_own_fp32_gradients(case_c):
    _, _, _, g64, g32, l32 = case_c
    assert len(g64) == 407 and set(g64) == set(g32)
    r = T.compare(g32, g64, g32)
    assert not r["bad"] and len(r["rows"]) == 407 - sum(T.is_bias_family(n) for n in g64)
    assert r["worst"][0] <= 1.0 / 3 + 1e-9                    # err == noise here, so err / (3e-4 + 3 noise) < 1/3
    assert r["n_loose"] <= 20
    T.check_losses({k: v.item() for k, v in l32.items()}, l32)
    with pytest.raises(AssertionError):
        T.check_losses({k: v.item() * (1 + 3e-4) for k, v in l32.items()}, l32)


def test_compare_reports_a_dropped_sample(seeded_sd, case_c):
    """The gradient of the first four samples alone, scaled by 4/5: what a kernel that skips the last sample's rows would return."""
    from test_oracle_golden import oracle_param_grads
    batch, noise, _, g64, g32, _ = case_c
    sb, nz = T.sub_batch(batch, noise, 0, 4)
    g4, _ = oracle_param_grads(seeded_sd, sb, nz)
    wrong = {n: g * 0.8 for n, g in g4.items()}
    r = T.compare(wrong, g64, g32, strict=False)
    assert len(r["bad"]) > 200 and r["worst"][0] > 10, (len(r["bad"]), r["worst"])
    with pytest.raises(AssertionError):
        T.compare(wrong, g64, g32)


def test_compare_reports_an_unmasked_padding_residue(seeded_sd, case_c):
    """res_mask of sample 1 (length 31) with one more true row: the mask-leak class of bug."""
    from test_oracle_golden import oracle_param_grads
    batch, noise, _, g64, g32, _ = case_c
    leak = dict(batch)
    leak["res_mask"] = batch["res_mask"].clone()
    assert not leak["res_mask"][1, 31] and leak["res_mask"][1, 30]
    leak["res_mask"][1, 31] = True
    wrong, _ = oracle_param_grads(seeded_sd, leak, noise)
    r = T.compare(wrong, g64, g32, strict=False)
    assert len(r["bad"]) > 50 and r["worst"][0] > 3, (len(r["bad"]), r["worst"])


def test_compare_reports_a_zeroed_row_block_of_one_weight_gradient(case_c):
    """One 16-row block of one [192,192] EdgeTransition weight gradient zeroed (a tile that was never written)."""
    _, _, _, g64, g32, _ = case_c
    name = "ga_encoder.trunk.edge_transition_2.trunk.2.weight"
    assert tuple(g64[name].shape) == (192, 192)
    for blk in (0, 5, 11):
        wrong = dict(g32)
        wrong[name] = g32[name].clone()
        wrong[name][16 * blk:16 * blk + 16] = 0
        r = T.compare(wrong, g64, g32, strict=False)
        assert _names(r) == {name}, (blk, r["bad"])


def test_compare_reports_a_transposed_gradient(case_c):
    """An initial_embed.weight gradient ([64,128]) transposed and laid back into its shape: same elements, same norm, wrong places."""
    _, _, _, g64, g32, _ = case_c
    name = "ga_encoder.trunk.edge_transition_0.initial_embed.weight"
    wrong = dict(g32)
    wrong[name] = g32[name].t().contiguous().reshape(g32[name].shape)
    assert torch.allclose(wrong[name].norm(), g32[name].norm())
    r = T.compare(wrong, g64, g32, strict=False)
    assert _names(r) == {name}, r["bad"]


def test_compare_reports_missing_misshapen_and_non_finite_gradients(case_c):
    _, _, _, g64, g32, _ = case_c
    names = sorted(n for n in g64 if not T.is_bias_family(n))
    wrong = dict(g32)
    del wrong[names[0]]
    wrong[names[1]] = g32[names[1]].reshape(-1)[:-1]
    wrong[names[2]] = g32[names[2]].clone()
    wrong[names[2]].view(-1)[0] = float("nan")
    bias = next(n for n in g64 if T.is_bias_family(n))
    wrong[bias] = torch.full_like(g32[bias], 1e-4)
    assert _names(T.compare(wrong, g64, g32, strict=False)) == {names[0], names[1], names[2], bias}
