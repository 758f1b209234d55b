"""GPU checks of the sequence kernels (csrc/seqalign.hip) through geometry.sequence_ratio / sequence_align / sequence_search: the
ratio, the match counts and the matching blocks EQUAL to difflib's (the ratio bit-equal: both sides are one IEEE float64 division of
the same integers), every integer output and x2y of the alignment equal to the plain-Python oracle (seq_oracle.py) in both modes, for
two matrices and two gap settings, the search equal to the argmax of the alignment over the Q x D pair list; bitwise repeatability,
independence of the work list's order and of its other pairs, fill values, the empty work list, the pairwise wrappers, clustering on
1 - identity, and metrics.sequence_scores after a short sample() run.  The cases are in seq_cases.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import seq_cases as SC  # noqa: E402
import seq_oracle as SO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import sequence_ratio  # noqa: E402,F401  (absent before this feature: every test here fails without it)

ALIGN_INTS = ("score", "n_ident", "n_aligned", "n_columns", "x_lo", "x_hi", "y_lo", "y_hi", "len_x", "len_y")


def cu(t):
    return torch.as_tensor(t).cuda()


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def batches():
    return {name: SC.make_batch(name) for name, _, _ in SC.BATCHES}


def ratio_of(b, pairs, **kw):
    aa, m = cu(b["aa"]), cu(b["mask"])
    return geometry.sequence_ratio(aa, aa, m, m, cu(pairs), **kw)


def align_of(b, pairs, **kw):
    aa, m = cu(b["aa"]), cu(b["mask"])
    if kw.get("matrix") is not None:
        kw["matrix"] = cu(kw["matrix"])
    return geometry.sequence_align(aa, aa, m, m, cu(pairs), **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the ratio ---------------------------------------------------------------------------------------------------------------------

def check_ratio(b, pairs, got):
    for p, (i, j) in enumerate(pairs.tolist()):
        where = (b["name"], p, i, j)
        if not SC.pair_ok(b, i, j):
            assert math.isnan(got["ratio"][p]) and got["matches"][p] == -1 and got["total"][p] == -1 and got["n_blocks"][p] == -1, where
            assert (got["blocks"][p] == np.array([-1, -1, 0])).all(), where
            continue
        x, y = b["seqs"][i], b["seqs"][j]
        blocks, matches, ratio = SO.difflib_blocks(x, y)
        assert (got["matches"][p], got["total"][p], got["len_x"][p], got["len_y"][p]) == (matches, len(x) + len(y), len(x), len(y)), where
        assert got["ratio"][p] == ratio and same_bits(got["ratio"][p:p + 1], np.array([ratio])), where      # bit-equal, no tolerance
        n = got["n_blocks"][p]
        assert n == len(blocks) and [tuple(r) for r in got["blocks"][p, :n].tolist()] == blocks, where
        assert (got["blocks"][p, n:] == np.array([-1, -1, 0])).all(), where


@pytest.mark.parametrize("P", SC.PAIR_COUNTS)
def test_ratio_equals_difflib(batches, P):
    for b in batches.values():
        pairs = SC.make_pairs(b, P)
        out = ratio_of(b, pairs, blocks=True)
        assert out["ratio"].dtype == torch.float64 and out["blocks"].shape == (P, 64, 3) and out["matches"].dtype == torch.int32
        check_ratio(b, pairs, host(out))


def test_ratio_of_every_pair_of_a_batch(batches):
    for b in batches.values():
        B = len(b["seqs"])
        pairs = np.stack(np.meshgrid(np.arange(B), np.arange(B), indexing="ij"), -1).reshape(-1, 2).astype(np.int32)
        check_ratio(b, pairs, host(ratio_of(b, pairs, blocks=True)))


# ---- the alignment -----------------------------------------------------------------------------------------------------------------

def check_align(b, pairs, got, matrix, gaps, mode):
    for p, (i, j) in enumerate(pairs.tolist()):
        where = (b["name"], p, i, j, matrix, gaps, mode)
        if not SC.pair_ok(b, i, j):
            assert got["score"][p] == SO.INT_MIN and math.isnan(got["identity"][p]) and (got["x2y"][p] == -1).all(), where
            assert all(got[k][p] == -1 for k in ALIGN_INTS[1:8]), where
            continue
        o = SC.align_oracle(b, i, j, matrix, gaps, mode)
        x, y = b["seqs"][i], b["seqs"][j]
        want = dict(o, len_x=len(x), len_y=len(y))
        assert {k: int(got[k][p]) for k in ALIGN_INTS} == {k: want[k] for k in ALIGN_INTS}, where
        assert got["x2y"][p].tolist() == o["x2y"] + [-1] * (64 - len(x)), where
        if o["n_columns"]:
            assert got["identity"][p] == o["n_ident"] / o["n_columns"], where              # one float64 division of the same integers
        else:
            assert math.isnan(got["identity"][p]), where


@pytest.mark.parametrize("gaps", SC.GAPS)
@pytest.mark.parametrize("matrix", sorted(SC.MATRICES))
@pytest.mark.parametrize("mode", SC.MODES)
def test_align_equals_the_oracle(batches, mode, matrix, gaps):
    counts = [P for P in SC.PAIR_COUNTS if P]
    for k, b in enumerate(batches.values()):
        pairs = SC.make_pairs(b, counts[(k + len(mode) + gaps[0]) % len(counts)])
        out = align_of(b, pairs, mode=mode, matrix=SC.MATRICES[matrix](), gap_open=gaps[0], gap_extend=gaps[1], alignment=True)
        assert out["identity"].dtype == torch.float64 and out["x2y"].shape == (len(pairs), 64) and out["score"].dtype == torch.int32
        check_align(b, pairs, host(out), matrix, gaps, mode)


def test_align_default_matrix_and_every_pair_count(batches):
    b = batches["n65_four"]
    for P in SC.PAIR_COUNTS:
        pairs = SC.make_pairs(b, P, seed=3)
        out = align_of(b, pairs, alignment=True)                            # match_matrix(), gap_open 2, gap_extend 1, global
        assert out["score"].shape == (P,)
        check_align(b, pairs, host(out), "match", (2, 1), "global")


# ---- the search --------------------------------------------------------------------------------------------------------------------

def library(D, Ld=40, letters=4, seed=2):
    rng = np.random.default_rng(seed + D)
    db_aa = rng.integers(0, letters, (D, Ld)).astype(np.int64)
    db_len = rng.choice(np.array([0, 1, 3, 7, 25, Ld]), D).astype(np.int32)
    for d in range(2, D, 5):                                # duplicated entries: equal scores, the lowest index wins
        db_aa[d], db_len[d] = db_aa[d - 2], db_len[d - 2]
    return db_aa, db_len


@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("D", (0, 1, 65, 300))
def test_search_is_the_argmax_of_the_alignment(batches, D, mode):
    b = batches["n65_four"]                                 # one query of 65 residues among them
    db_aa, db_len = library(D)
    Q, N = b["aa"].shape
    kw = dict(mode=mode, matrix=cu(SC.random_matrix()), gap_open=3, gap_extend=1)
    got = host(geometry.sequence_search(cu(b["aa"]), cu(b["mask"]), cu(db_aa), cu(db_len), **kw))
    assert got["best_index"].dtype == np.int32 and got["best_identity"].dtype == np.float64
    long_q = np.array([len(s) > 64 for s in b["seqs"]])
    if D == 0:
        assert (got["best_index"] == -1).all() and (got["best_score"] == SO.INT_MIN).all() and np.isnan(got["best_identity"]).all()
        return
    # the device's own alignment over the whole Q x D list: queries as x, library entries as y, padded to a common N
    W = max(N, db_aa.shape[1])
    aa_q, m_q = np.zeros((Q, W), np.int64), np.zeros((Q, W), bool)
    aa_q[:, :N], m_q[:, :N] = b["aa"], b["mask"]
    aa_d, m_d = np.zeros((D, W), np.int64), np.zeros((D, W), bool)
    aa_d[:, :db_aa.shape[1]] = db_aa
    m_d[:, :db_aa.shape[1]] = np.arange(db_aa.shape[1])[None] < db_len[:, None]
    pairs = np.stack(np.meshgrid(np.arange(Q), np.arange(D), indexing="ij"), -1).reshape(-1, 2).astype(np.int32)
    al = host(geometry.sequence_align(cu(aa_q), cu(aa_d), cu(m_q), cu(m_d), cu(pairs), **kw))
    score = al["score"].reshape(Q, D).astype(np.int64)
    best = score.argmax(1)                                  # numpy's argmax: the first of equal maxima
    ties = 0
    for q in range(Q):
        if long_q[q]:
            assert got["best_index"][q] == -1 and got["best_score"][q] == SO.INT_MIN and got["best_n_ident"][q] == -1
            assert got["best_n_columns"][q] == -1 and math.isnan(got["best_identity"][q])
            continue
        p = q * D + best[q]
        assert (got["best_index"][q], got["best_score"][q]) == (best[q], score[q, best[q]]), q
        assert (got["best_n_ident"][q], got["best_n_columns"][q]) == (al["n_ident"][p], al["n_columns"][p]), q
        assert same_bits(got["best_identity"][q:q + 1], al["identity"][p:p + 1]), q
        ties += int((score[q] == score[q, best[q]]).sum() > 1)
    assert D < 65 or ties > 0                               # the duplicated entries did tie
    # and the plain-Python oracle on a few queries
    lib = [db_aa[d, :db_len[d]].tolist() for d in range(D)]
    some = [q for q in range(Q) if len(b["seqs"][q]) <= 7][:4] + [int(np.flatnonzero(long_q)[0])]
    want = SO.search([b["seqs"][q] for q in some], lib, SC.random_matrix(), 3, 1, mode)
    for q, w in zip(some, want):
        assert (got["best_index"][q], got["best_score"][q], got["best_n_ident"][q], got["best_n_columns"][q]) == w, q


# ---- properties --------------------------------------------------------------------------------------------------------------------

def test_repeatable_and_independent_of_the_work_list(batches):
    b = batches["n144_twenty"]
    pairs = SC.make_pairs(b, 257)
    kw = dict(mode="local", matrix=SC.random_matrix(), gap_open=2, gap_extend=1, alignment=True)
    r1, r2 = host(ratio_of(b, pairs, blocks=True)), host(ratio_of(b, pairs, blocks=True))
    a1, a2 = host(align_of(b, pairs, **kw)), host(align_of(b, pairs, **kw))
    for one, two in ((r1, r2), (a1, a2)):
        for k in one:
            assert same_bits(one[k], two[k]), k
    perm = np.random.default_rng(0).permutation(len(pairs))
    rp, ap = host(ratio_of(b, pairs[perm], blocks=True)), host(align_of(b, pairs[perm], **kw))
    for one, two in ((r1, rp), (a1, ap)):
        for k in one:
            assert same_bits(one[k][perm], two[k]), k
    more = np.concatenate([SC.make_pairs(b, 65, seed=9), pairs, SC.make_pairs(b, 63, seed=8)])
    rm, am = host(ratio_of(b, more, blocks=True)), host(align_of(b, more, **kw))
    for one, two in ((r1, rm), (a1, am)):
        for k in one:
            assert same_bits(one[k], two[k][65:65 + len(pairs)]), k
    db_aa, db_len = library(65)
    s = [host(geometry.sequence_search(cu(b["aa"]), cu(b["mask"]), cu(db_aa), cu(db_len))) for _ in range(2)]
    for k in s[0]:
        assert same_bits(s[0][k], s[1][k]), k


def test_fill_values_leave_the_neighbours_intact(batches):
    b = batches["n65_four"]
    B = len(b["seqs"])
    long_row = next(i for i, s in enumerate(b["seqs"]) if len(s) == 65)
    good = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [5, 2]], np.int32)
    bad = np.array([[long_row, 1], [-1, 3], [4, B], [6, long_row], [B + 7, -2]], np.int32)
    mixed = np.stack([good, bad], 1).reshape(-1, 2)         # good, bad, good, bad, ...
    for run in (lambda pp: host(ratio_of(b, pp, blocks=True)), lambda pp: host(align_of(b, pp, mode="local", alignment=True))):
        alone, among = run(good), run(mixed)
        for k in alone:
            assert same_bits(alone[k], among[k][0::2]), k
    r, a = host(ratio_of(b, bad, blocks=True)), host(align_of(b, bad, alignment=True))
    assert np.isnan(r["ratio"]).all() and (r["matches"] == -1).all() and (r["n_blocks"] == -1).all() and (r["total"] == -1).all()
    assert (a["score"] == SO.INT_MIN).all() and np.isnan(a["identity"]).all() and (a["n_columns"] == -1).all() and (a["x2y"] == -1).all()
    # the lengths are reported where the indices are good, also above the bound
    assert r["len_x"].tolist() == a["len_x"].tolist() == [65, -1, -1, len(b["seqs"][6]), -1]
    assert r["len_y"].tolist() == a["len_y"].tolist() == [len(b["seqs"][1]), -1, -1, 65, -1]


def test_empty_work_list_launches_nothing(batches):
    b = batches["n64_two"]
    from pepflowww_amd import _capi
    calls = _capi.CALLS
    r, a = ratio_of(b, np.zeros((0, 2), np.int32), blocks=True), align_of(b, np.zeros((0, 2), np.int32), alignment=True)
    assert _capi.CALLS == calls
    assert r["ratio"].shape == (0,) and r["blocks"].shape == (0, 64, 3) and a["x2y"].shape == (0, 64) and a["score"].shape == (0,)
    db_aa, db_len = library(1)
    s = geometry.sequence_search(cu(b["aa"][:0]), cu(b["mask"][:0]), cu(db_aa), cu(db_len))
    assert _capi.CALLS == calls and s["best_index"].shape == (0,)


# ---- the pairwise wrappers and the metrics driver ----------------------------------------------------------------------------------

def test_pairwise_wrappers_and_clustering(batches):
    b = batches["n64_two"]
    keep = [i for i, s in enumerate(b["seqs"]) if len(s) > 0]
    aa, m = cu(b["aa"][keep]), cu(b["mask"][keep])
    seqs = [b["seqs"][i] for i in keep]
    B = len(keep)
    groups = torch.tensor([0, 1] * (B // 2) + [0] * (B % 2))
    ratio = geometry.pairwise_sequence_ratio(aa, m, groups=groups)
    ident = geometry.pairwise_sequence_identity(aa, m, groups=groups, mode="global", gap_open=3, gap_extend=3)
    torch.cuda.synchronize()
    assert ratio.dtype == torch.float64 and ratio.shape == (B, B) and ident.shape == (B, B)
    for i in range(B):
        for j in range(B):
            if i == j:
                assert ratio[i, j] == 1.0 and ident[i, j] == 1.0
            elif groups[i] != groups[j]:
                assert math.isnan(ratio[i, j]) and math.isnan(ident[i, j])
            else:
                lo, hi = min(i, j), max(i, j)               # the direction kept: a = sequence i, b = sequence j with i < j
                assert ratio[i, j].item() == SO.difflib_blocks(seqs[lo], seqs[hi])[2]
                o = SO.align(seqs[lo], seqs[hi], SC.match_matrix(), 3, 3)
                assert ident[i, j].item() == o["n_ident"] / o["n_columns"]
    full = geometry.pairwise_sequence_identity(aa, m)
    cl = geometry.cluster(1.0 - full, 0.4, method="complete")
    torch.cuda.synchronize()
    label = cl["label"].cpu().numpy()
    d = (1.0 - full).float().cpu().numpy()
    assert label.shape == (B,) and int(cl["n_clusters"][0]) == label.max() + 1
    for i in range(B):                                      # complete linkage cut at 0.4: every pair inside a cluster is within it
        for j in range(B):
            assert label[i] != label[j] or d[i, j] <= np.float32(0.4)


def test_sequence_scores_after_a_short_sample(seeded_sd):
    dev = torch.device("cuda:0")
    model = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    model.load_state_dict(seeded_sd)
    model = model.to(dev).eval()
    B, L, NS = 4, 24, 2
    batch = synth.make_pocket_batch(B, L, 7, seed=4)
    final = model.sample({k: v.to(dev) for k, v in batch.items()}, num_steps=NS, noise=synth.make_noise(B, L, NS, seed=6))[-1]
    groups = torch.tensor([0, 0, 0, 1])
    gen = batch["generate_mask"].bool()
    rng = np.random.default_rng(1)
    db_aa = torch.as_tensor(rng.integers(0, 20, (30, 12)))
    db_len = torch.as_tensor(rng.integers(1, 13, 30))
    native = [SO.compact(final["seqs_1"][s].cpu().tolist(), gen[s].tolist()) for s in range(B)]
    db_aa[17, :len(native[0][:12])] = torch.tensor(native[0][:12])
    out = metrics.sequence_scores(final, batch, groups=groups, known=(db_aa, db_len))
    torch.cuda.synchronize()
    sample = [SO.compact(final["seqs"][s].cpu().tolist(), gen[s].tolist()) for s in range(B)]
    for s in range(B):
        assert len(sample[s]) == 7 and out["seq_ratio"][s].item() == SO.difflib_blocks(sample[s], native[s])[2]
        o = SO.align(sample[s], native[s], SC.match_matrix(), 2, 1)
        assert out["align_identity"][s].item() == o["n_ident"] / o["n_columns"]
        same = sum(a == c for a, c in zip(sample[s], native[s]))
        assert abs(out["aar"][s].item() - same / len(native[s])) < 1e-6      # fp32 quotient of two small integers
    pr = [SO.difflib_blocks(sample[i], sample[j])[2] for i in range(3) for j in range(i + 1, 3)]
    assert abs(out["diversity_seq"][0].item() - (1.0 - sum(pr) / 3)) < 1e-12 and math.isnan(out["diversity_seq"][1].item())
    assert out["group_labels"].tolist() == [0, 1]
    lib = [db_aa[d, :int(db_len[d])].tolist() for d in range(30)]
    want = SO.search(sample, lib, SC.match_matrix(), 2, 1)
    assert out["nearest_known"].tolist() == [w[0] for w in want]
    for s, w in enumerate(want):
        assert out["nearest_identity"][s].item() == w[2] / w[3]
    assert out["novel_seq"].tolist() == [w[2] / w[3] < 0.5 for w in want] and out["novel_seq"].dtype == torch.bool
