"""CPU checks of the sequence ratio, alignment and search: the alignment oracle (seq_oracle.py) against the brute-force enumeration of
every alignment, the returned alignment re-scored by hand, the restated block rules the kernel follows against difflib itself, the
ctypes struct layouts against the header, the exported symbols, and the wrappers' argument checks."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import seq_cases as SC  # noqa: E402
import seq_oracle as SO  # noqa: E402
from pepflowww_amd import _capi, build, geometry, metrics  # noqa: E402
from test_lddt_cpu import header_fields  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pepflow_hip.h")


def short_sequences(max_len=4, letters=2):
    return [list(s) for n in range(max_len + 1) for s in itertools.product(range(letters), repeat=n)]


# ---- the alignment oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("matrix", sorted(SC.MATRICES))
def test_alignment_oracle_against_every_alignment(mode, matrix):
    m = SC.MATRICES[matrix]()
    seqs = short_sequences()
    for go, ge in ((3, 1), (2, 2), (1, 0)):                 # gap_open != gap_extend among them
        for x in seqs:
            for y in seqs:
                o = SO.align(x, y, m, go, ge, mode)
                assert o["score"] == SO.brute_force(x, y, m, go, ge, mode), (x, y, go, ge)
                # the returned alignment, re-scored by hand, is worth the score and covers the span
                assert SO.score_columns(x, y, o["columns"], m, go, ge) == o["score"]
                xs = [a for a, _ in o["columns"] if a >= 0]
                ys = [b for _, b in o["columns"] if b >= 0]
                assert xs == list(range(o["x_lo"], o["x_hi"])) and ys == list(range(o["y_lo"], o["y_hi"]))
                assert o["n_columns"] == len(o["columns"]) >= o["n_aligned"] >= o["n_ident"]
                if mode == "global":
                    assert (o["x_lo"], o["x_hi"], o["y_lo"], o["y_hi"]) == (0, len(x), 0, len(y))
                else:
                    assert o["score"] >= 0 and (o["score"] > 0 or o["n_columns"] == 0)


def test_alignment_oracle_hand_cases():
    m = SC.match_matrix()
    # one gap of two: 4 matches - (2 + 1)
    o = SO.align([0, 1, 2, 3], [0, 1, 5, 6, 2, 3], m, 2, 1)
    assert o["score"] == 1 and o["x2y"] == [0, 1, 4, 5] and (o["n_ident"], o["n_aligned"], o["n_columns"]) == (4, 4, 6)
    # local: the common core, nothing else
    o = SO.align([9, 9, 0, 1, 2, 8], [7, 0, 1, 2], m, 2, 1, "local")
    assert o["score"] == 3 and (o["x_lo"], o["x_hi"], o["y_lo"], o["y_hi"]) == (2, 5, 1, 4) and o["x2y"] == [-1, -1, 1, 2, 3, -1]
    # ties: the diagonal before F before E -- with equal scores the traceback takes the mismatch column, not two gaps
    o = SO.align([0], [1], m, 1, 0)
    assert o["score"] == -1 and o["columns"] == [(0, 0)]
    # empty sides
    assert SO.align([], [], m, 2, 1)["score"] == 0 and SO.align([], [1, 2, 3], m, 2, 1)["score"] == -4
    assert SO.align([], [1, 2, 3], m, 2, 1)["n_columns"] == 3 and SO.align([1], [], m, 2, 1, "local")["n_columns"] == 0


# ---- the ratio's description against difflib ---------------------------------------------------------------------------------------

def test_restated_block_rules_are_difflibs():
    rng = np.random.default_rng(11)
    n = 0
    for letters in (1, 2, 3, 4, 20):
        for _ in range(400):
            a = rng.integers(0, letters, rng.integers(0, 65)).tolist()
            b = rng.integers(0, letters, rng.integers(0, 65)).tolist()
            blocks, matches, ratio = SO.difflib_blocks(a, b)
            assert SO.restated_blocks(a, b) == (blocks, matches, ratio), (a, b)
            n += ratio != SO.difflib_blocks(b, a)[2]
    assert n > 0                                            # the ratio depends on the direction
    for name, _, _ in SC.BATCHES:
        seqs = [s for s in SC.make_batch(name)["seqs"] if len(s) <= SO.MAX_LEN]
        for a in seqs:
            for b in seqs:
                assert SO.restated_blocks(a, b) == SO.difflib_blocks(a, b)


def test_cases_cover_what_they_claim():
    lengths, padded = set(), set()
    for name, N, _ in SC.BATCHES:
        b = SC.make_batch(name)
        lengths |= {len(s) for s in b["seqs"]}
        padded.add(N)
        if N >= 65:                                         # a 64-residue row that crosses the chunk edge
            assert any(len(s) == 64 and b["mask"][i, 64:].any() and b["mask"][i, :64].any() for i, s in enumerate(b["seqs"]))
        pairs = SC.make_pairs(b, 65)
        assert (pairs == -1).any() and (pairs == len(b["seqs"])).any()
    assert lengths >= set(SC.LENGTHS) | {65} and padded == set(SC.PADDED)
    assert any(t == 20 for s in SC.make_batch("n144_twenty")["seqs"] for t in s)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("struct,cls", [("pf_seq_ratio_args", _capi.SeqRatioArgs), ("pf_seq_align_args", _capi.SeqAlignArgs),
                                        ("pf_seq_search_args", _capi.SeqSearchArgs)])
def test_struct_layout_agrees_with_the_header(struct, cls):
    assert [(n, t) for n, t in cls._fields_] == header_fields(struct)
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0


def test_header_source_list_and_symbols():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("int pf_polar_fwd(") < text.index("} pf_seq_ratio_args;") < text.index("} pf_seq_align_args;") \
        < text.index("} pf_seq_search_args;") < text.index("} pf_lddt_args;")
    for name, value in (("PF_SEQ_MAX_LEN", geometry.SEQ_MAX_LEN), ("PF_SEQ_TYPES", geometry.SEQ_TYPES), ("PF_SEQ_MAX_GAP", geometry.SEQ_MAX_GAP)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value
    assert (geometry.SEQ_MAX_LEN, geometry.SEQ_TYPES) == (SO.MAX_LEN, SO.TYPES) and geometry.SEQ_INT_MIN == SO.INT_MIN
    assert geometry.SEQ_MODES == ("global", "local") and "#define PF_SEQ_GLOBAL 0" in text and "#define PF_SEQ_LOCAL 1" in text
    assert "seqalign.hip" in build.SOURCES
    syms = _capi.EXPORTED_SYMBOLS
    k = syms.index("pf_seq_ratio_fwd")
    assert syms[k:k + 3] == ("pf_seq_ratio_fwd", "pf_seq_align_fwd", "pf_seq_search_fwd")


def test_library_exports_the_entry_points():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION
    for fn, cls in ((lib.pf_seq_ratio_fwd, _capi.SeqRatioArgs), (lib.pf_seq_align_fwd, _capi.SeqAlignArgs),
                    (lib.pf_seq_search_fwd, _capi.SeqSearchArgs)):
        assert fn(None, None) == -1 and fn(C.byref(cls()), None) == -1


# ---- the wrappers' argument checks, before any device work -------------------------------------------------------------------------

def test_wrapper_argument_checks():
    aa, m = torch.zeros(3, 8, dtype=torch.int64), torch.ones(3, 8, dtype=torch.bool)
    pairs = torch.tensor([[0, 1]])
    for f in (geometry.sequence_ratio, geometry.sequence_align):
        for bad in ((aa[:, :7], aa, m, m), (aa, aa, m[:2], m), (aa, aa, m, m[:, :7]), (aa.float(), aa, m, m), (aa[0], aa, m, m),
                    (aa[:, :0], aa[:, :0], m[:, :0], m[:, :0])):
            with pytest.raises(ValueError):
                f(*bad, pairs)
        with pytest.raises(ValueError):
            f(aa, aa, m, m, torch.tensor([0, 1]))
    for kw in (dict(mode="semiglobal"), dict(gap_open=1, gap_extend=2), dict(gap_extend=-1), dict(gap_open=4097), dict(gap_open=1.5),
               dict(matrix=torch.zeros(20, 20, dtype=torch.int64)), dict(matrix=torch.zeros(21, 21)),
               dict(matrix=torch.full((21, 21), 128)), dict(matrix=torch.full((21, 21), -129))):
        with pytest.raises(ValueError):
            geometry.sequence_align(aa, aa, m, m, pairs, **kw)
        with pytest.raises(ValueError):
            geometry.sequence_search(aa, m, aa, torch.tensor([8, 8, 8]), **kw)
    db = torch.zeros(3, 8, dtype=torch.int64)
    for bad in ((aa, m[:2], db, torch.tensor([1, 2, 3])), (aa, m, db, torch.tensor([1, 2])), (aa, m, torch.zeros(3, 65, dtype=torch.int64), torch.tensor([1, 2, 3])),
                (aa, m, db.float(), torch.tensor([1, 2, 3])), (aa, m, db[:, :0], torch.tensor([0, 0, 0]))):
        with pytest.raises(ValueError):
            geometry.sequence_search(*bad)
    mm = geometry.match_matrix(2, -3)
    assert mm.dtype == torch.int8 and tuple(mm.shape) == (21, 21) and int(mm[20, 20]) == 2 and int(mm[0, 20]) == -3
    assert np.array_equal(geometry.match_matrix().numpy(), SC.match_matrix())
    # no CPU path: tensors on the host are refused, not computed
    with pytest.raises(_capi.PepflowHipError):
        geometry.sequence_ratio(aa, aa, m, m, pairs)
    assert callable(metrics.sequence_scores)
