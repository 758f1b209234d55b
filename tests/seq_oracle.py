"""Host oracles of the sequence kernels (csrc/seqalign.hip), plain Python.

  ratio       difflib.SequenceMatcher(None, a, b) itself, over strings made from the type bytes (`difflib_blocks`); `restated_blocks`
              is the description the kernel follows (window match, tie-breaking, explicit stack, merge), kept here so that the CPU
              suite can hold the description against difflib.
  alignment   `align`: Gotoh's recurrences and the traceback's tie rules as the head of csrc/seqalign.hip states them, on Python integers; `brute_force`
              enumerates every alignment of two short sequences and is what `align` is held against.
Sequences are lists of types 0..20 (20: X)."""
import difflib

INT_MIN = -2 ** 31
NEG = INT_MIN // 2          # "minus infinity" of the recurrences
MAX_LEN = 64
TYPES = 21


def compact(aa_row, mask_row):
    """the types of a padded row where the mask is set, in order; a type outside 0..19 is 20"""
    return [int(t) if 0 <= int(t) <= 19 else 20 for t, m in zip(aa_row, mask_row) if m]


def as_string(seq):
    return "".join(chr(65 + t) for t in seq)


# ---- the ratio ---------------------------------------------------------------------------------------------------------------------

def difflib_blocks(a, b):
    """-> (blocks without the sentinel, matches, ratio) of difflib on the two sequences"""
    sm = difflib.SequenceMatcher(None, as_string(a), as_string(b))
    blocks = [tuple(m) for m in sm.get_matching_blocks()[:-1]]
    return blocks, sum(k for _, _, k in blocks), sm.ratio()


def window_match(a, b, alo, ahi, blo, bhi):
    """the longest common substring inside the window; of equal lengths the smallest start in a, then the smallest start in b"""
    best = (0, alo, blo)
    for i in range(alo, ahi):
        for j in range(blo, bhi):
            k = 0
            while i + k < ahi and j + k < bhi and a[i + k] == b[j + k]:
                k += 1
            if k > best[0]:                       # i, then j ascend: the first of equal lengths stays
                best = (k, i, j)
    return best[1], best[2], best[0]


def restated_blocks(a, b):
    """the rules of csrc/seqalign.hip: explicit stack, at most 2 * 64 + 1 windows, blocks sorted and adjacent ones merged"""
    stack, found = [], []
    if a and b:
        stack.append((0, len(a), 0, len(b)))
    for _ in range(2 * MAX_LEN + 1):
        if not stack:
            break
        alo, ahi, blo, bhi = stack.pop()
        i, j, k = window_match(a, b, alo, ahi, blo, bhi)
        if k:
            found.append((i, j, k))
            if alo < i and blo < j:
                stack.append((alo, i, blo, j))
            if i + k < ahi and j + k < bhi:
                stack.append((i + k, ahi, j + k, bhi))
    assert not stack
    merged = []
    for i, j, k in sorted(found):
        if merged and merged[-1][0] + merged[-1][2] == i and merged[-1][1] + merged[-1][2] == j:
            merged[-1] = (merged[-1][0], merged[-1][1], merged[-1][2] + k)
        else:
            merged.append((i, j, k))
    matches, total = sum(k for _, _, k in merged), len(a) + len(b)
    return merged, matches, (2.0 * matches / total if total else 1.0)


# ---- the alignment -----------------------------------------------------------------------------------------------------------------

def align(x, y, matrix, gap_open, gap_extend, mode="global"):
    """-> dict(score, n_ident, n_aligned, n_columns, x_lo, x_hi, y_lo, y_hi, x2y [len x], columns): the recurrences

         E[i][j] = max(V[i][j-1] - gap_open, E[i][j-1] - gap_extend)        a column of y against a gap
         F[i][j] = max(V[i-1][j] - gap_open, F[i-1][j] - gap_extend)        a column of x against a gap
         V[i][j] = max(V[i-1][j-1] + s, F[i][j], E[i][j])                   local: max(0, ...)

    with the traceback's ties fixed: at V the diagonal first, then F, then E; inside E and F "opened here" before "extended".
    columns: the alignment as (i, j) per column, -1 for a gap, in order."""
    lx, ly, local = len(x), len(y), mode == "local"
    V = [[NEG] * (ly + 1) for _ in range(lx + 1)]
    E = [[NEG] * (ly + 1) for _ in range(lx + 1)]
    F = [[NEG] * (ly + 1) for _ in range(lx + 1)]
    V[0][0] = 0
    for j in range(1, ly + 1):
        V[0][j] = 0 if local else -gap_open - (j - 1) * gap_extend
        E[0][j] = V[0][j]
    for i in range(1, lx + 1):
        V[i][0] = 0 if local else -gap_open - (i - 1) * gap_extend
        F[i][0] = V[i][0]
    for i in range(1, lx + 1):
        for j in range(1, ly + 1):
            E[i][j] = max(V[i][j - 1] - gap_open, E[i][j - 1] - gap_extend)
            F[i][j] = max(V[i - 1][j] - gap_open, F[i - 1][j] - gap_extend)
            v = max(V[i - 1][j - 1] + int(matrix[x[i - 1]][y[j - 1]]), F[i][j], E[i][j])
            V[i][j] = max(0, v) if local else v
    if local:
        score, i, j = 0, 0, 0
        for ii in range(1, lx + 1):               # the largest cell; of equal cells the smallest i, then the smallest j
            for jj in range(1, ly + 1):
                if V[ii][jj] > score:
                    score, i, j = V[ii][jj], ii, jj
    else:
        score, i, j = V[lx][ly], lx, ly
    x_hi, y_hi = i, j
    cols, state = [], "V"
    while i > 0 or j > 0:
        if local and state == "V" and V[i][j] == 0:
            break
        if i == 0 or j == 0:                      # global: the end gap that is left
            assert not local and state == "V"
            if i:
                cols.append((i - 1, -1))
                i -= 1
            else:
                cols.append((-1, j - 1))
                j -= 1
            continue
        if state == "V":
            if V[i][j] == V[i - 1][j - 1] + int(matrix[x[i - 1]][y[j - 1]]):
                cols.append((i - 1, j - 1))
                i, j = i - 1, j - 1
                continue
            state = "F" if V[i][j] == F[i][j] else "E"
            assert state == "F" or V[i][j] == E[i][j]
        if state == "F":
            state = "V" if F[i][j] == V[i - 1][j] - gap_open else "F"
            cols.append((i - 1, -1))
            i -= 1
        else:
            state = "V" if E[i][j] == V[i][j - 1] - gap_open else "E"
            cols.append((-1, j - 1))
            j -= 1
    cols.reverse()
    x2y = [-1] * lx
    for a, b in cols:
        if a >= 0 and b >= 0:
            x2y[a] = b
    return dict(score=score, n_ident=sum(1 for a, b in cols if a >= 0 and b >= 0 and x[a] == y[b]),
                n_aligned=sum(1 for a, b in cols if a >= 0 and b >= 0), n_columns=len(cols),
                x_lo=i if local else 0, x_hi=x_hi, y_lo=j if local else 0, y_hi=y_hi, x2y=x2y, columns=cols)


def score_columns(x, y, cols, matrix, gap_open, gap_extend):
    """the score of an alignment given as columns, by hand: substitution scores minus gap_open + (g - 1) gap_extend per gap run"""
    total, run = 0, None                          # run: which side the current gap run is on
    for a, b in cols:
        if a >= 0 and b >= 0:
            total += int(matrix[x[a]][y[b]])
            run = None
        else:
            side = "x" if b < 0 else "y"
            total -= gap_extend if run == side else gap_open
            run = side
    return total


def _global_alignments(lx, ly):
    """every global alignment of sequences of lx and ly letters as a list of columns"""
    if lx == 0 and ly == 0:
        yield []
        return
    if lx and ly:
        for rest in _global_alignments(lx - 1, ly - 1):
            yield rest + [(lx - 1, ly - 1)]
    if lx:
        for rest in _global_alignments(lx - 1, ly):
            yield rest + [(lx - 1, -1)]
    if ly:
        for rest in _global_alignments(lx, ly - 1):
            yield rest + [(-1, ly - 1)]


_BRUTE = {}          # global brute-force scores by (x, y, matrix bytes, gap_open, gap_extend)


def brute_force(x, y, matrix, gap_open, gap_extend, mode="global"):
    """the best score over every alignment (global), or over every alignment of every pair of substrings and the empty one (local)"""
    if mode == "global":
        key = (tuple(x), tuple(y), bytes(memoryview(matrix)), gap_open, gap_extend)
        if key not in _BRUTE:
            _BRUTE[key] = max(score_columns(x, y, c, matrix, gap_open, gap_extend) for c in _global_alignments(len(x), len(y)))
        return _BRUTE[key]
    best = 0
    for x0 in range(len(x) + 1):
        for x1 in range(x0, len(x) + 1):
            for y0 in range(len(y) + 1):
                for y1 in range(y0, len(y) + 1):
                    best = max(best, brute_force(x[x0:x1], y[y0:y1], matrix, gap_open, gap_extend))
    return best


def search(queries, library, matrix, gap_open, gap_extend, mode="global"):
    """-> per query (index, score, n_ident, n_columns) of the library entry with the highest score, lowest index of equal scores;
    (-1, INT_MIN, -1, -1) for an empty library or a query above 64 residues"""
    res = []
    for q in queries:
        best = (-1, INT_MIN, -1, -1)
        if len(q) <= MAX_LEN:
            for d, e in enumerate(library):
                o = align(q, e, matrix, gap_open, gap_extend, mode)
                if best[0] < 0 or o["score"] > best[1]:
                    best = (d, o["score"], o["n_ident"], o["n_columns"])
        res.append(best)
    return res
