"""The block-level checker (tests/block_oracle.py) is sound and catches what it is for -- CPU oracle only, no kernel involved.

Every case reaches its gate margins within the round limit; the three block functions are the pieces ga_encoder is made of; the
oracle's own fp32 gradients pass the rule in every case and region; and a wrong tensor built from the truth, one class of kernel bug
at a time, is reported with the region it sits in.  The lines that are wrong on purpose live only here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from oracle import pepflow_oracle as O  # noqa: E402
import block_oracle as K  # noqa: E402
import train_oracle as T  # noqa: E402

ALL = [(kind, name) for kind in ("ipa", "node", "et") for name in K.CASES[kind]]
_TRUTH = {}


def _truth(sd, kind, name):
    if (kind, name) not in _TRUTH:
        _TRUTH[(kind, name)] = K.truth(sd, kind, name)
    return _TRUTH[(kind, name)]


def test_cases_are_the_listed_shapes():
    for kind, cases in K.CASES.items():
        for name, (B, L, lengths, hole) in cases.items():
            mask = K.case_mask(B, L, lengths, hole)
            assert mask.shape == (B, L) and mask.sum(1).tolist() == [n - (hole is not None and b == 0) for b, n in enumerate(lengths)], (kind, name)
            assert (mask < 0.5).any(), (kind, name)            # every case has masked rows: the truth's zero is checked on them
    B, L, lengths, _ = K.CASES["node"]["65x64"]
    assert lengths[0] == 64 and min(lengths) >= 40 and max(lengths) == 64 and len(lengths) == 65
    # the extra case whose launch tail (rows % 4, pairs % 64) is made of REAL rows and pairs
    mask = K.case_mask(*K._TAIL_REAL)
    assert {n for n, _ in K.regions(mask, False)} >= {"launch-tail"} and {n for n, _ in K.regions(mask, True)} >= {"launch-tail"}


@pytest.mark.parametrize("kind,name", ALL)
def test_case_reaches_its_margins_and_the_reference_passes_the_rule(seeded_sd, kind, name):
    """The gate margin holds (>= 5 x the oracle's fp32 miss, within 20 rounds), the float64 truth is zero on masked rows and pairs
    (asserted by K.truth), and the oracle's own fp32 gradients pass `compare` in every region, its parameter gradients
    train_oracle.compare."""
    tr = _truth(seeded_sd, kind, name)
    m = tr["margins"]
    K.assert_margins(m)
    assert m["rounds"] <= K.MAX_ROUNDS and m["margin"] >= K.MARGIN_FACTOR * m["miss"]
    if K.GATES[kind]:
        assert 0 < m["miss"] < 1e-4, m             # an fp32 forward of one block misses a pre-activation by a few 1e-6
    r = K.compare(tr, tr["act32"], masked_zero=tuple(tr["act64"]))
    assert {n for n, *_ in r["rows"]} == set(K.GRAD_NAMES[kind])
    assert r["worst"][0] < 1 / K.K_NOISE                # err == noise here, so err / (REL + 3 noise) < 1 / 3
    p = K.compare_params(tr, tr["par32"])
    assert len(p["rows"]) + sum(T.is_bias_family(n) for n in tr["par64"]) == len(K.block_params(seeded_sd, kind, K.BLOCK))
    noise, where = max((n, (t, reg)) for t, reg, _, n, _ in r["rows"])
    print(f"{kind} {name}: margin {m['margin']:.2e} (required {m['required']:.2e}, fp32 miss {m['miss']:.2e}), rounds {m['rounds']}, "
          f"re-drawn {m['redrawn']}; oracle fp32 noise on the activation gradients <= {noise:.2e} ({where[0]}, {where[1]}), on the parameters worst err/tol {p['worst'][0]:.3f}")
    # the rule's noise term stays of the order of REL at most (measured 3e-7 .. 2e-6; 6.5e-5 for g_trans of IPA where the launch tail
    # is ONE row, a cancelling sum normalised by its own three entries)
    assert noise < 3 * K.REL, noise


def test_block_functions_are_the_pieces_of_ga_encoder(seeded_sd):
    """Chained on ga_encoder's own s, z, R, x entering block 0 at (3, 23), the three block functions reproduce its ln_in_0, s_0, z_0."""
    B, L, lengths, n_gen, seed = T.GRID["a"]
    batch, noise = T.make_case(B, L, lengths, n_gen, seed)
    sd = seeded_sd
    with torch.no_grad():
        enc = O.encode(sd, batch)
        t, R_t, x_t, ang_t, seq_t = O.corrupt(batch, enc, noise)
        col = {}
        O.ga_encoder(sd, t, R_t, x_t, ang_t, seq_t, enc[4], enc[5], batch["res_mask"].long(), collect=col)
        mask = batch["res_mask"].float()
        ln_in = col["s_in"] + K.ipa_fn(sd, 0, mask)(col["s_in"], enc[5], R_t.float(), x_t)
        s0 = K.node_fn(sd, 0, mask)(ln_in)
        z0 = K.et_fn(sd, 0, mask)(s0, enc[5])
    for got, key in ((ln_in, "ln_in_0"), (s0, "s_0"), (z0, "z_0")):
        assert (got - col[key]).abs().max() <= 1e-6 * col[key].abs().max().clamp_min(1.0), key


def _bad(tr, got, **kw):
    r = K.compare(tr, got, strict=False, **kw)
    return {(n, reg) for n, reg, *_ in r["bad"]}, r


def test_planted_errors_are_reported_with_their_region(seeded_sd):
    tr = _truth(seeded_sd, "ipa", "77")
    B, L, lengths, _ = K.CASES["ipa"]["77"]
    clean = lambda: {k: v.clone() for k, v in tr["act64"].items()}
    assert not _bad(tr, clean())[0]
    # the last 16-key chunk of one query row of g_z scaled by 1.01.  The rule resolves 1e-4 of a region's maximum, so the row is the
    # one that holds the largest entry of that chunk (1 % of it is then 1e-2 of the column band's maximum)
    g = clean()
    n1 = lengths[1]
    i = int(g["g_z"][1, :, n1 - 16:n1].abs().amax((1, 2)).argmax())
    g["g_z"][1, i, n1 - 16:n1] *= 1.01
    bad, r = _bad(tr, g)
    assert ("g_z", "colband 1") in bad and ("g_z", "colband 0") not in bad and not any(n != "g_z" for n, _ in bad), bad
    assert f"worst at [1, {i}," in next(d for n, reg, _, _, d in r["bad"] if reg == "colband 1")
    # the last real row of the last sample of g_s shifted by 1e-3 of the tensor maximum
    g = clean()
    g["g_s"][B - 1, lengths[-1] - 1] += 1e-3 * g["g_s"].abs().max()
    bad, _ = _bad(tr, g)
    assert ("g_s", f"tail {B - 1}") in bad and ("g_s", "tail 0") not in bad and ("g_s", "whole") in bad, bad
    # g_trans of one row changes sign
    g = clean()
    g["g_trans"][0, 30] *= -1
    bad, _ = _bad(tr, g)
    assert ("g_trans", "sample 0") in bad and ("g_trans", "sample 1") not in bad and ("g_trans", "tail 0") not in bad, bad
    # one masked pair of g_z set to NaN
    g = clean()
    g["g_z"][1, 3, L - 1, 7] = float("nan")
    bad, _ = _bad(tr, g)
    assert bad == {("g_z", "masked")}, bad
    # a masked row that is finite but not zero: reported only where a consumer reads it unmasked
    g = clean()
    g["g_s"][1, L - 1] = 1.0
    assert not _bad(tr, g)[0] and _bad(tr, g, masked_zero=("g_s",))[0] == {("g_s", "masked")}
    # a missing tensor
    g = clean()
    del g["g_rot"]
    assert ("g_rot", "-") in _bad(tr, g)[0]


@pytest.mark.parametrize("kind", ["ipa", "node", "et"])
def test_zeroed_launch_tail_is_reported(seeded_sd, kind):
    """The last rows % 4 rows (pairs % 64 pairs) of the launch zeroed, at the case whose last sample is the full one."""
    tr = _truth(seeded_sd, kind, "23-tail")
    for name, g64 in tr["act64"].items():
        g = {k: v.clone() for k, v in tr["act64"].items()}
        flat = g[name].reshape(-1, g64.shape[-1])
        k = 64 if K.is_pair(g64) else 4
        assert flat.shape[0] % k
        flat[flat.shape[0] // k * k:] = 0
        bad, _ = _bad(tr, g)
        assert (name, "launch-tail") in bad and all(n == name for n, _ in bad), (name, bad)
