"""Seeded cases of the sequence kernels, shared by the CPU and the GPU tests.

A batch is aa [B,N] / mask [B,N] with the set residues SCATTERED over the N slots (so that the device's compaction crosses its 64-slot
chunk edge for N = 65 and 144).  Lengths are drawn from LENGTHS, every one of them at least once where N allows it; alphabets of 1, 2
and 4 letters produce the ties (in windows and in tracebacks) that 20 letters almost never do.  Batches with N >= 65 carry one row of
65 set residues (above PF_SEQ_MAX_LEN: fill values); the 20-letter batch carries types outside 0..19 (X).  Work lists draw pairs with
repetition and, from 3 pairs on, hold an index of -1 and one of B."""
import numpy as np

import seq_oracle as SO

LENGTHS = (0, 1, 2, 3, 7, 25, 63, 64)
PADDED = (1, 64, 65, 144)
PAIR_COUNTS = (0, 1, 63, 64, 65, 257)
# (name, N, letters)
BATCHES = (("n1", 1, 2), ("n64_two", 64, 2), ("n64_one", 64, 1), ("n65_four", 65, 4), ("n144_twenty", 144, 20))
GAPS = ((2, 1), (3, 3))             # (gap_open, gap_extend): affine, and linear (every tie between "opened" and "extended")
MODES = ("global", "local")


def make_batch(name):
    _, N, letters = next(b for b in BATCHES if b[0] == name)
    rng = np.random.default_rng(sum(name.encode()) * 7919 + N)
    lengths = [n for n in LENGTHS if n <= N]
    lengths += [int(rng.choice(lengths)) for _ in range(max(0, 10 - len(lengths)))]
    if N >= 65:
        lengths.append(65)
    B = len(lengths)
    aa = rng.integers(0, letters, (B, N)).astype(np.int64)
    if letters == 20:                                       # types outside 0..19 are X, and X equals X
        odd = rng.random((B, N)) < 0.08
        aa[odd] = rng.choice(np.array([20, 21, 25, -1, -7, 1 << 40]), int(odd.sum()))
    mask = np.zeros((B, N), bool)
    for b, n in enumerate(lengths):
        mask[b, np.sort(rng.choice(N, n, replace=False))] = True
    seqs = [SO.compact(aa[b], mask[b]) for b in range(B)]
    assert [len(s) for s in seqs] == lengths
    return dict(name=name, N=N, aa=aa, mask=mask, seqs=seqs)


def make_pairs(batch, P, seed=0):
    B = batch["aa"].shape[0]
    rng = np.random.default_rng(1000 * P + seed + batch["N"])
    pairs = rng.integers(0, B, (P, 2)).astype(np.int32)
    if P >= 3:
        pairs[P // 3, 0] = -1
        pairs[(2 * P) // 3, 1] = B
    return pairs


def pair_ok(batch, i, j):
    """whether the pair gets a result (else: the fill values)"""
    B = len(batch["seqs"])
    return 0 <= i < B and 0 <= j < B and len(batch["seqs"][i]) <= SO.MAX_LEN and len(batch["seqs"][j]) <= SO.MAX_LEN


def random_matrix(seed=5):
    """a seeded asymmetric [21,21] matrix with small entries (many equal scores), diagonal mostly positive"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-3, 3, (SO.TYPES, SO.TYPES))
    m[np.arange(SO.TYPES), np.arange(SO.TYPES)] = rng.integers(0, 5, SO.TYPES)
    assert (m != m.T).any()
    return m.astype(np.int64)


def match_matrix(match=1, mismatch=-1):
    m = np.full((SO.TYPES, SO.TYPES), mismatch, np.int64)
    np.fill_diagonal(m, match)
    return m


MATRICES = {"match": match_matrix, "random": random_matrix}

_ALIGN_CACHE = {}


def align_oracle(batch, i, j, matrix_name, gaps, mode):
    """seq_oracle.align of rows i and j of the batch, computed once per (batch, pair, setting)"""
    key = (batch["name"], i, j, matrix_name, gaps, mode)
    if key not in _ALIGN_CACHE:
        _ALIGN_CACHE[key] = SO.align(batch["seqs"][i], batch["seqs"][j], MATRICES[matrix_name](), gaps[0], gaps[1], mode)
    return _ALIGN_CACHE[key]
