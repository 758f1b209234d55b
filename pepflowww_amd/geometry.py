"""Evaluation geometry on the device: thin wrappers that check their arguments, bind device pointers into one argument struct and
launch one HIP entry point each (the kernels and their conventions are described in csrc/*.hip).

Input families, one binding path each:
  pair work lists   point sets x [Bx,N,3] / y [By,N,3] with masks and `pairs` [P,2] -- `_pair_inputs`: superpose (and align, batch_align,
                    superpose_rmsd), tm_score, tm_align and their pairwise_* matrices (`_within_groups`, `_mirrored`);
  heavy-atom structures   pos [B,N,A,3], atom_mask [B,N,A] and per-residue [B,N] tensors -- `_structure`: structural_violations, sasa,
                    torsion_angles, interface_energy, polar_interactions, pack_sidechains, mutation_scan and each side of sidechain_compare (dssp reads the same pos with a residue mask);
                    cavity_scan (pf_cavity_fwd: buriedness scan, cavities and lining residues of whole receptors, N <= 4096) too;
  both at once      two heavy-atom structure sets and a work list -- `_structure_pairs`: lddt (pf_lddt_fwd, the values of OpenFold's
                    lddt / lddt_ca, openfold/utils/loss.py:382-458) and interface_contacts (pf_contacts_fwd), which dockq combines
                    with `superpose` into Fnat, iRMSD, LRMSD and DockQ.
  distance matrices a [B,B] device matrix of one of the pairwise_* functions and host group labels -- `cluster` (pf_cluster_fwd): gromos
                    and single / complete / average linkage clusters of the samples of each group, their representatives and the
                    best-scored member of each.  The linkages are checked against scipy's fcluster(criterion="distance"), as
                    partitions only; gromos follows the publication (Daura et al. 1999) and is not checked against GROMACS.
  sequences         residue types aa [B,N] with masks and `pairs` [P,2] -- `_seq_pair_inputs`: sequence_ratio (pf_seq_ratio_fwd: difflib's
                    SequenceMatcher ratio, the reference's diff_ratio), sequence_align (pf_seq_align_fwd: Gotoh, global / local, a caller's
                    matrix) and their pairwise_sequence_* matrices; sequence_search (pf_seq_search_fwd) against a compact library.
`_bind_in` / `_bind_out` fill the struct, `_as_bool` turns the byte outputs into bool, `_table` keeps the per-device constant tables.

Deviation from the reference: `batch_align` selects each sample's masked atoms on their own.  The reference's
`masked_select(...).reshape(B, -1, 3)` mixes atoms across samples when the per-sample mask counts differ; where the counts are equal
the results are the same."""
import ctypes as C
import math

import torch

from . import _capi

_TABLES = {}


def _table(name, dev, make, *key):
    """the constant table `name` on `dev`, built by make() (a CPU tensor) on first use; key: what else it depends on (n_points)"""
    k = (name, str(dev)) + key
    if k not in _TABLES:
        _TABLES[k] = make().contiguous().to(dev)
    return _TABLES[k]


def _f32(t, dev):
    return t.to(dev, torch.float32).contiguous()


def _bytes(t, dev):
    """a mask as uint8 on the device; a bool tensor is reinterpreted, not copied"""
    t = t.to(dev)
    return (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).contiguous()


def _bind_in(a, **tensors):
    """device pointers of the inputs into the argument struct `a` (None: the field stays null); a CPU tensor raises, no fallback"""
    for k, t in tensors.items():
        if t is not None:
            setattr(a, k, _capi.dptr(t, t.dtype, k))


def _bind_out(a, out):
    for k, t in out.items():
        setattr(a, k, t.data_ptr())


def _as_bool(out, *keys):
    """the byte outputs among `keys` that are there, as bool (the kernels write 0 / 1: a reinterpretation)"""
    for k in keys:
        if k in out:
            out[k] = out[k].view(torch.bool)


def _check_pairs(pairs):
    pairs = torch.as_tensor(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"pairs must be [P,2], got {tuple(pairs.shape)}")
    return pairs


def _pair_inputs(a, name, x, y, mx, my, pairs, max_n=None, nonempty=False):
    """The pair-work-list family: checks x [Bx,N,3], y [By,N,3], mx [Bx,N], my [By,N], pairs [P,2] (ValueError), N <= max_n
    (PepflowHipError, before any device work) and, with `nonempty`, that neither side is empty; converts (y is x and my is mx share
    one buffer) and binds x, y, mx, my, pairs, Bx, By, N, P into `a`.  -> (the tensors to keep alive, device, N, P)"""
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"x must be [B,N,3], got {tuple(x.shape)}")
    Bx, N, _ = x.shape
    By = y.shape[0] if y.dim() == 3 else -1
    if tuple(y.shape[1:]) != (N, 3) or tuple(mx.shape) != (Bx, N) or tuple(my.shape) != (By, N):
        raise ValueError(f"shapes do not agree: x {tuple(x.shape)}, y {tuple(y.shape)}, mx {tuple(mx.shape)}, my {tuple(my.shape)}")
    pairs = _check_pairs(pairs)
    if max_n is not None and N > max_n:
        raise _capi.PepflowHipError(f"{name}: N = {N} points exceeds the kernel's bound of {max_n}")
    if nonempty and (N == 0 or Bx == 0 or By == 0):
        raise ValueError(f"{name} needs at least one point set of at least one point on each side")
    dev = x.device
    kx, kmx = _f32(x, dev), _bytes(mx, dev)
    keep = [kx, kx if y is x else _f32(y, dev), kmx, kmx if my is mx else _bytes(my, dev), pairs.to(dev, torch.int32).contiguous()]
    _bind_in(a, x=keep[0], y=keep[1], mx=keep[2], my=keep[3], pairs=keep[4])
    a.Bx, a.By, a.N, a.P = Bx, By, N, pairs.shape[0]
    return keep, dev, N, pairs.shape[0]


def _within_groups(B, groups):
    """-> pairs [P,2] int32: every i < j of the same group (all one group when `groups` is None)"""
    return group_pairs(torch.zeros(B, dtype=torch.int64) if groups is None else groups)[0]


def _mirrored(B, pairs, dev, *filled):
    """one [B,B] matrix per (values [P], diagonal) of `filled`: values at (i, j) and (j, i) of each pair, NaN elsewhere"""
    i, j = pairs[:, 0].to(dev, torch.int64), pairs[:, 1].to(dev, torch.int64)
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    res = []
    for v, diag in filled:
        m = torch.full((B, B), float("nan"), device=dev)
        m[i, j] = v
        m[j, i] = v
        res.append(m.masked_fill(eye, diag))
    return res


def _structure(pos, atom_mask, per_residue, max_n=None, tag="", dev=None):
    """The heavy-atom family: checks pos [B,N,A,3] (A >= 14), atom_mask [B,N,A] and the [B,N] tensors of per_residue = ((name, tensor
    or None, dtype), ...), and N <= max_n (ValueError); converts pos to float32, atom_mask to bytes and each given tensor to its
    dtype (uint8: a mask), on `dev` (None: where pos is).
    -> (device, (B, N, A), pos, atom_mask, [the converted per-residue tensors, None where not given])"""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 4 or pos.shape[3] != 3 or pos.shape[2] < VIOLATION_SLOTS:
        raise ValueError(f"{tag}pos must be [B,N,A,3] with A >= {VIOLATION_SLOTS}, got {tuple(getattr(pos, 'shape', ()))}")
    B, N, A, _ = pos.shape
    if tuple(atom_mask.shape) != (B, N, A):
        raise ValueError(f"{tag}atom_mask must be [B,N,A] = {(B, N, A)}, got {tuple(atom_mask.shape)}")
    for nm, t, _ in per_residue:
        if t is not None and tuple(t.shape) != (B, N):
            raise ValueError(f"{tag}{nm} must be [B,N] = {(B, N)}, got {tuple(t.shape)}")
    if max_n is not None and N > max_n:
        raise ValueError(f"at most {max_n} residues per structure, got {N}")
    dev = pos.device if dev is None else dev
    conv = [None if t is None else _bytes(t, dev) if dt is torch.uint8 else t.to(dev, dt).contiguous() for _, t, dt in per_residue]
    return dev, (B, N, A), _f32(pos, dev), _bytes(atom_mask, dev), conv


def superpose(x, y, mx, my, pairs, aa_x=None, aa_y=None, allow_reflection=False, transform=False, aligned=False):
    """pf_superpose_fwd over the work list `pairs` [P,2] (pair p = (i, j): x[i] onto y[j] on the points mx[i] & my[j]).

    x [Bx,N,3], y [By,N,3] (y may be x), mx [Bx,N], my [By,N], aa_x / aa_y [B.,N] int64 (optional, both or neither).
    -> dict of device tensors: rmsd_plain, rmsd (proper Kabsch), count, degenerate [P]; ident [P] if aa_x is given; rot [P,3,3],
    trans [P,3] if `transform`; aligned [P,N,3] (rot x[i] + trans for all N points) if `aligned`.  rot / trans / aligned follow
    `allow_reflection` (True: the reference's `align` rotation, which may be a reflection; False: the proper rotation)."""
    if (aa_x is None) != (aa_y is None):
        raise ValueError("aa_x and aa_y go together")
    a = _capi.SuperposeArgs()
    keep, dev, N, P = _pair_inputs(a, "superpose", x, y, mx, my, pairs)
    out = {"rmsd_plain": torch.empty(P, device=dev), "rmsd": torch.empty(P, device=dev),
           "count": torch.empty(P, dtype=torch.int32, device=dev), "degenerate": torch.empty(P, dtype=torch.uint8, device=dev)}
    if aa_x is not None:
        keep.append(aa_x.to(dev, torch.int64).reshape(a.Bx, N).contiguous())
        keep.append(keep[-1] if aa_y is aa_x else aa_y.to(dev, torch.int64).reshape(a.By, N).contiguous())
        _bind_in(a, aa_x=keep[-2], aa_y=keep[-1])
        out["ident"] = torch.empty(P, device=dev)
    if transform:
        out["rot"], out["trans"] = torch.empty(P, 3, 3, device=dev), torch.empty(P, 3, device=dev)
    if aligned:
        out["aligned"] = torch.empty(P, N, 3, device=dev)
    _bind_out(a, out)
    a.allow_reflection = int(bool(allow_reflection))
    if P:
        _capi.check(_capi.load().pf_superpose_fwd(C.byref(a), _capi.stream_ptr()), "pf_superpose_fwd")
    _as_bool(out, "degenerate")
    return out


def batch_align(pos_1, pos_2, pos_mask):
    """(B,L,A,3), (B,L,A,3), (B,L,A) -> (pos_1 aligned onto pos_2, pos_2).  The reference's rule: r = V U^T from the SVD of
    S = X^T Y over the masked atoms (no determinant correction: a mirror image is aligned by a reflection), applied with its
    translation to every atom of pos_1, masked ones included."""
    B, L, A, _ = pos_1.shape
    ids = torch.arange(B, device=pos_1.device, dtype=torch.int32)
    out = superpose(pos_1.reshape(B, L * A, 3), pos_2.reshape(B, L * A, 3), pos_mask.reshape(B, L * A), pos_mask.reshape(B, L * A),
                    torch.stack([ids, ids], 1), allow_reflection=True, aligned=True)
    return out["aligned"].reshape(B, L, A, 3).to(pos_1.dtype), pos_2


def align(pos_1, pos_2, pos_mask):
    """(L,A,3), (L,A,3), (L,A) -> (pos_1 aligned onto pos_2, pos_2): `batch_align` of one sample."""
    aligned, _ = batch_align(pos_1[None], pos_2[None], pos_mask[None])
    return aligned[0], pos_2


def superpose_rmsd(x, y, mask):
    """x, y [B,N,3], mask [B,N] -> [B]: RMSD after the optimal proper rotation and translation of x[b] onto y[b] (Kabsch;
    Biopython's Superimposer.rms).  NaN where the mask is empty."""
    ids = torch.arange(x.shape[0], device=x.device, dtype=torch.int32)
    return superpose(x, y, mask, mask, torch.stack([ids, ids], 1))["rmsd"]


def group_pairs(groups):
    """groups [B] (any integer labels) -> (pairs [P,2] int32 of every i < j with the same label, group index [P] into `labels`,
    labels [G] sorted).  Index plumbing on the host."""
    groups = torch.as_tensor(groups).reshape(-1).cpu()
    labels, inv = torch.unique(groups, sorted=True, return_inverse=True)
    i, j = torch.triu_indices(groups.numel(), groups.numel(), offset=1)
    same = inv[i] == inv[j]
    pairs = torch.stack([i[same], j[same]], 1).to(torch.int32)
    return pairs, inv[i[same]], labels


def pairwise_superpose_rmsd(x, mask, aa=None, groups=None):
    """x [B,N,3], mask [B,N] -> rmsd [B,B]: proper Kabsch RMSD of every pair i < j of the same group (all one group when `groups`
    is None), mirrored, so the matrix is exactly symmetric with an exact-zero diagonal; pairs across groups are NaN.
    With `aa` [B,N] -> (rmsd, ident [B,B]): the fraction of the shared points with the same residue type (diagonal 1)."""
    B = x.shape[0]
    pairs = _within_groups(B, groups)
    out = superpose(x, x, mask, mask, pairs, aa_x=aa, aa_y=aa)
    if aa is None:
        return _mirrored(B, pairs, x.device, (out["rmsd"], 0.0))[0]
    return tuple(_mirrored(B, pairs, x.device, (out["rmsd"], 0.0), (out["ident"], 1.0)))


TM_MAX_N = 512              # PF_TM_MAX_N: the longest point set pf_tm_score_fwd takes
TM_SLOT_BYTES = 112         # PF_TM_SLOT_BYTES: one scratch slot (the best candidate of 64 seeds)


def tm_score(x, y, mx, my, pairs, transform=False, aligned=False):
    """pf_tm_score_fwd over the work list `pairs` [P,2]: TM-score of x[i] against y[j] with the residue correspondence fixed
    (the TMscore program's algorithm, Zhang & Skolnick 2004), on the points mx[i] & my[j], normalised by the target's count my[j].

    x [Bx,N,3], y [By,N,3] (y may be x), mx [Bx,N], my [By,N], N <= TM_MAX_N.
    -> dict of device tensors: tm [P] (NaN where fewer than 3 points are shared), count [P] (shared points; 0 for pair indices out
    of range), lnorm [P] (the normalising count); rot [P,3,3], trans [P,3] of the best superposition (y ~ rot x + trans, a proper
    rotation) if `transform`; aligned [P,N,3] (rot x[i] + trans for all N points) if `aligned`."""
    a = _capi.TmScoreArgs()
    keep, dev, N, P = _pair_inputs(a, "tm_score", x, y, mx, my, pairs, max_n=TM_MAX_N, nonempty=True)
    out = {"tm": torch.empty(P, device=dev), "count": torch.empty(P, dtype=torch.int32, device=dev),
           "lnorm": torch.empty(P, dtype=torch.int32, device=dev)}
    if transform:
        out["rot"], out["trans"] = torch.empty(P, 3, 3, device=dev), torch.empty(P, 3, device=dev)
    if aligned:
        out["aligned"] = torch.empty(P, N, 3, device=dev)
    _bind_out(a, out)
    if P:
        lib = _capi.load()
        keep.append(torch.empty(P * lib.pf_tm_score_work_slots(N) * TM_SLOT_BYTES, dtype=torch.uint8, device=dev))
        a.work = keep[-1].data_ptr()
        _capi.check(lib.pf_tm_score_fwd(C.byref(a), _capi.stream_ptr()), "pf_tm_score_fwd")
    return out


def pairwise_tm_score(x, mask, groups=None):
    """x [B,N,3], mask [B,N] -> tm [B,B]: TM-score of every pair i < j of the same group (all one group when `groups` is None), x[i]
    onto x[j] normalised by mask[j], mirrored, so the matrix is exactly symmetric with a diagonal of 1; pairs across groups are NaN.
    Within a group of one complex the masks are equal and the score does not depend on the direction."""
    B = x.shape[0]
    pairs = _within_groups(B, groups)
    return _mirrored(B, pairs, x.device, (tm_score(x, x, mask, mask, pairs)["tm"], 1.0))[0]


TM_ALIGN_MAX_N = 512        # PF_TM_ALIGN_MAX_N: the most slots pf_tm_align_fwd takes


def tm_align(x, y, mx, my, pairs, transform=False, alignment=False, aligned=False, max_len=None):
    """pf_tm_align_fwd: TM-align (Zhang & Skolnick 2005) of chain 1 = x[i] on mx[i] (the model) onto chain 2 = y[j] on my[j] (the
    target) for every pair (i, j) of `pairs` [P,2]: a sequence-independent alignment of the CA traces, in fp64 on the device.  The
    conventions are listed in csrc/tm_align.hip.

    x [Bx,N,3], y [By,N,3] (y may be x), mx [Bx,N], my [By,N], N <= TM_ALIGN_MAX_N.  max_len: an optional upper bound on the
    unmasked counts, which sizes the kernel's LDS (a 25-residue peptide in 256 slots needs only 25); a pair above it returns NaN and
    n_aligned -1.
    -> dict of device tensors, with tmtools' TMResult names alongside:
      tm [P]          normalised by chain 2's length Ly: tmtools' tm_norm_chain2 (what eval/geometry.py's get_tm returns);
      tm_x [P]        normalised by Lx: tm_norm_chain1;
      rmsd [P]        Kabsch RMSD of the n_aligned pairs: rmsd;
      n_aligned [P]   pairs within score_d8 after the final superposition (TM-align's n_ali8; -1 above max_len);
      len_x, len_y [P];
      rot [P,3,3], trans [P,3] (`transform`): the superposition of the search behind tm, y ~ rot x + trans -- tmtools' u, t
                      correspond to it, but which of the program's final searches tmtools copies out cannot be checked here;
      y2x [P,N] int32, kept [P,N] bool (`alignment`): for each y position the aligned x position (an index into N, -1 none) and
                      whether the pair counts in n_aligned; seqxA / seqyA follow from y2x;
      aligned [P,N,3] (`aligned`): rot x + trans for all N points.
    NaN scores where a chain has fewer than 3 residues or the pair indices are out of range (n_aligned 0)."""
    if max_len is not None and not (0 <= int(max_len)):
        raise ValueError(f"max_len must be >= 0, got {max_len}")
    a = _capi.TmAlignArgs()
    keep, dev, N, P = _pair_inputs(a, "tm_align", x, y, mx, my, pairs, max_n=TM_ALIGN_MAX_N, nonempty=True)
    out = {"tm": torch.empty(P, device=dev), "tm_x": torch.empty(P, device=dev), "rmsd": torch.empty(P, device=dev)}
    for k in ("n_aligned", "len_x", "len_y"):
        out[k] = torch.empty(P, dtype=torch.int32, device=dev)
    if transform:
        out["rot"], out["trans"] = torch.empty(P, 3, 3, device=dev), torch.empty(P, 3, device=dev)
    if alignment:
        out["y2x"], out["kept"] = torch.empty(P, N, dtype=torch.int32, device=dev), torch.empty(P, N, dtype=torch.uint8, device=dev)
    if aligned:
        out["aligned"] = torch.empty(P, N, 3, device=dev)
    _bind_out(a, out)
    a.max_len = 0 if max_len is None else min(int(max_len), N)
    if P:
        _capi.check(_capi.load().pf_tm_align_fwd(C.byref(a), _capi.stream_ptr()), "pf_tm_align_fwd")
    _as_bool(out, "kept")
    return out


def pairwise_tm_align(x, mask, groups=None):
    """x [B,N,3], mask [B,N] -> tm [B,B]: TM-align of every pair i < j of the same group (all one group when `groups` is None), x[i]
    onto x[j], normalised by chain j's length, mirrored as pairwise_tm_score is, with a diagonal of 1; pairs across groups are NaN.
    Unlike the fixed-correspondence TM-score, TM-align's score may depend on the direction; the i-onto-j one is kept."""
    B = x.shape[0]
    pairs = _within_groups(B, groups)
    max_len = int(torch.as_tensor(mask).bool().sum(1).max()) if B else 0
    return _mirrored(B, pairs, x.device, (tm_align(x, x, mask, mask, pairs, max_len=max_len)["tm"], 1.0))[0]


SEQ_MAX_LEN = 64            # PF_SEQ_MAX_LEN: the longest compacted sequence the pf_seq_* kernels take
SEQ_TYPES = 21              # PF_SEQ_TYPES: the 20 residue types and X (every type outside 0..19)
SEQ_MAX_GAP = 4096          # PF_SEQ_MAX_GAP
SEQ_MODES = ("global", "local")     # PF_SEQ_GLOBAL, PF_SEQ_LOCAL
SEQ_INT_MIN = -2 ** 31      # the fill value of a score


def match_matrix(match=1, mismatch=-1):
    """-> [21,21] int8 (CPU): `match` on the diagonal (X against X included), `mismatch` elsewhere.  The default scoring of
    sequence_align; no published substitution table is shipped, callers pass their own [21,21] matrix."""
    m = torch.full((SEQ_TYPES, SEQ_TYPES), int(mismatch), dtype=torch.int64)
    m.fill_diagonal_(int(match))
    return _check_matrix(m)


def _check_matrix(matrix):
    """-> the [21,21] integer matrix as int8 (where it is), entries in [-128, 127] (ValueError)"""
    if not isinstance(matrix, torch.Tensor) or tuple(matrix.shape) != (SEQ_TYPES, SEQ_TYPES):
        raise ValueError(f"matrix must be a [{SEQ_TYPES},{SEQ_TYPES}] tensor, got {tuple(getattr(matrix, 'shape', ()))}")
    if matrix.is_floating_point() or matrix.is_complex() or matrix.dtype == torch.bool:
        raise ValueError(f"matrix must hold integers, got {matrix.dtype}")
    if matrix.dtype != torch.int8:
        lo, hi = int(matrix.min()), int(matrix.max())
        if lo < -128 or hi > 127:
            raise ValueError(f"matrix entries must lie in [-128, 127], got [{lo}, {hi}]")
    return matrix.to(torch.int8)


def _seq_scoring(mode, matrix, gap_open, gap_extend):
    """checks the scoring arguments of sequence_align / sequence_search (ValueError, before any device work)
    -> bind(a, dev): sets them in the argument struct and returns the device matrix to keep alive"""
    if mode not in SEQ_MODES:
        raise ValueError(f"mode must be one of {SEQ_MODES}, got {mode!r}")
    if int(gap_open) != gap_open or int(gap_extend) != gap_extend or not 0 <= gap_extend <= gap_open <= SEQ_MAX_GAP:
        raise ValueError(f"gap penalties must be integers with 0 <= gap_extend <= gap_open <= {SEQ_MAX_GAP}, got {gap_open}, {gap_extend}")
    checked = None if matrix is None else _check_matrix(matrix)

    def bind(a, dev):
        m = (_table("seq_match_matrix", dev, match_matrix) if checked is None else checked.to(dev)).contiguous()
        _bind_in(a, matrix=m)
        a.mode, a.gap_open, a.gap_extend = SEQ_MODES.index(mode), int(gap_open), int(gap_extend)
        return m
    return bind


def _seq_pair_inputs(a, name, aa_x, aa_y, mx, my, pairs):
    """The pair-work-list family on residue types: checks aa_x, mx [Bx,N], aa_y, my [By,N], pairs [P,2] (ValueError), converts (aa_y is
    aa_x and my is mx share one buffer) and binds them with Bx, By, N, P into `a`.  -> (the tensors to keep alive, device, P)"""
    for nm, t in (("aa_x", aa_x), ("aa_y", aa_y), ("mx", mx), ("my", my)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: {nm} must be a [B,N] tensor, got {tuple(getattr(t, 'shape', ()))}")
    for nm, t in (("aa_x", aa_x), ("aa_y", aa_y)):
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"{name}: {nm} must hold integer residue types, got {t.dtype}")
    Bx, N = aa_x.shape
    By = aa_y.shape[0]
    if aa_y.shape[1] != N or tuple(mx.shape) != (Bx, N) or tuple(my.shape) != (By, N):
        raise ValueError(f"shapes do not agree: aa_x {tuple(aa_x.shape)}, aa_y {tuple(aa_y.shape)}, mx {tuple(mx.shape)}, my {tuple(my.shape)}")
    pairs = _check_pairs(pairs)
    if N == 0 or Bx == 0 or By == 0:
        raise ValueError(f"{name} needs at least one sequence slot of at least one residue on each side")
    dev = aa_x.device
    kx, kmx = aa_x.to(dev, torch.int64).contiguous(), _bytes(mx, dev)
    keep = [kx, kx if aa_y is aa_x else aa_y.to(dev, torch.int64).contiguous(), kmx, kmx if my is mx else _bytes(my, dev),
            pairs.to(dev, torch.int32).contiguous()]
    _bind_in(a, aa_x=keep[0], aa_y=keep[1], mx=keep[2], my=keep[3], pairs=keep[4])
    a.Bx, a.By, a.N, a.P = Bx, By, N, pairs.shape[0]
    return keep, dev, pairs.shape[0]


def sequence_ratio(aa_x, aa_y, mx, my, pairs, blocks=False):
    """pf_seq_ratio_fwd: difflib.SequenceMatcher(None, a, b).ratio() -- the reference's `diff_ratio` (eval/geometry.py) -- for every
    pair (i, j) of `pairs` [P,2], with a = the types aa_x[i] where mx[i] is set, in order, and b = aa_y[j] where my[j] is set.  The
    conventions (difflib's tie-breaking, no junk) are listed in csrc/seqalign.hip.

    aa_x [Bx,N], aa_y [By,N] integer residue types (a type outside 0..19 is X, and X equals X), mx [Bx,N], my [By,N]; N is not
    bounded, the sequences (the set residues) may have up to SEQ_MAX_LEN = 64 residues and may be empty.
    -> dict of device tensors: ratio [P] float64 = 2.0 * matches / total (1.0 when both are empty), bit-equal to difflib's;
    matches, total, len_x, len_y [P] int32; with `blocks`: blocks [P,64,3] int32, the (i, j, k) of get_matching_blocks() without its
    sentinel, unused rows (-1, -1, 0), and n_blocks [P].
    A sequence above 64 residues or a pair index out of range: ratio NaN, matches, total and n_blocks -1.  The ratio is not symmetric
    in (a, b)."""
    a = _capi.SeqRatioArgs()
    keep, dev, P = _seq_pair_inputs(a, "sequence_ratio", aa_x, aa_y, mx, my, pairs)
    out = {"ratio": torch.empty(P, dtype=torch.float64, device=dev)}
    for k in ("matches", "total", "len_x", "len_y"):
        out[k] = torch.empty(P, dtype=torch.int32, device=dev)
    if blocks:
        out["blocks"] = torch.empty(P, SEQ_MAX_LEN, 3, dtype=torch.int32, device=dev)
        out["n_blocks"] = torch.empty(P, dtype=torch.int32, device=dev)
    _bind_out(a, out)
    if P:
        _capi.check(_capi.load().pf_seq_ratio_fwd(C.byref(a), _capi.stream_ptr()), "pf_seq_ratio_fwd")
    return out


def sequence_align(aa_x, aa_y, mx, my, pairs, mode="global", matrix=None, gap_open=2, gap_extend=1, alignment=False):
    """pf_seq_align_fwd: Gotoh's affine-gap pairwise alignment of the sequences of every pair of `pairs` [P,2] (inputs as in
    `sequence_ratio`), in int32 on the device.  The recurrences and the traceback's tie rules are listed in csrc/seqalign.hip.

    mode: "global" (Needleman-Wunsch with penalised end gaps) or "local" (Smith-Waterman; of equal best cells the smallest x index,
    then the smallest y index).  matrix: [21,21] integers in [-128, 127], matrix[x type][y type] (None: match_matrix(), +1 / -1);
    no substitution table is shipped.  A gap of length g costs gap_open + (g - 1) gap_extend, 0 <= gap_extend <= gap_open <= 4096.
    -> dict of device tensors [P]: score, n_ident (columns of equal types), n_aligned (columns without a gap), n_columns, x_lo,
    x_hi, y_lo, y_hi (the aligned span [lo, hi) in the compacted sequences; the whole sequences in global mode), len_x, len_y int32;
    identity float64 = n_ident / n_columns (needle's / water's definition; NaN without columns -- the counts are there for another
    denominator); with `alignment`: x2y [P,64] int32, the y index aligned to the k-th residue of x (-1: a gap or outside the span).
    A sequence above 64 residues or a pair index out of range: score SEQ_INT_MIN, the counts and the span -1, identity NaN."""
    a = _capi.SeqAlignArgs()
    scoring = _seq_scoring(mode, matrix, gap_open, gap_extend)
    keep, dev, P = _seq_pair_inputs(a, "sequence_align", aa_x, aa_y, mx, my, pairs)
    keep.append(scoring(a, dev))
    out = {k: torch.empty(P, dtype=torch.int32, device=dev)
           for k in ("score", "n_ident", "n_aligned", "n_columns", "x_lo", "x_hi", "y_lo", "y_hi", "len_x", "len_y")}
    out["identity"] = torch.empty(P, dtype=torch.float64, device=dev)
    if alignment:
        out["x2y"] = torch.empty(P, SEQ_MAX_LEN, dtype=torch.int32, device=dev)
    _bind_out(a, out)
    if P:
        _capi.check(_capi.load().pf_seq_align_fwd(C.byref(a), _capi.stream_ptr()), "pf_seq_align_fwd")
    return out


def sequence_search(aa, mask, db_aa, db_len, mode="global", matrix=None, gap_open=2, gap_extend=1):
    """pf_seq_search_fwd: for each query (the types aa[q] where mask[q] is set; aa, mask [Q,N]) the entry of the library with the
    highest `sequence_align` score, of equal scores the lowest index -- "the closest known peptide".  db_aa [D,Ld] integer types,
    already compact (entry d is db_aa[d, :db_len[d]]), Ld <= 64; db_len [D]; an entry whose length is outside [0, Ld] is never the
    best.  mode / matrix / gap_open / gap_extend as in `sequence_align`.  The Q x D scores are never stored: one workgroup per query.
    -> dict of device tensors [Q]: best_index, best_score, best_n_ident, best_n_columns int32, best_identity float64.
    A query above 64 residues, or an empty library: best_index -1, best_score SEQ_INT_MIN, the counts -1, best_identity NaN."""
    for nm, t in (("aa", aa), ("mask", mask), ("db_aa", db_aa)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"sequence_search: {nm} must be a 2-d tensor, got {tuple(getattr(t, 'shape', ()))}")
    for nm, t in (("aa", aa), ("db_aa", db_aa)):
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"sequence_search: {nm} must hold integer residue types, got {t.dtype}")
    Q, N = aa.shape
    D, Ld = db_aa.shape
    db_len = torch.as_tensor(db_len)
    if tuple(mask.shape) != (Q, N) or tuple(db_len.shape) != (D,):
        raise ValueError(f"shapes do not agree: aa {tuple(aa.shape)}, mask {tuple(mask.shape)}, db_aa {tuple(db_aa.shape)}, "
                         f"db_len {tuple(db_len.shape)}")
    if N == 0:
        raise ValueError("sequence_search needs query slots of at least one residue")
    if not 1 <= Ld <= SEQ_MAX_LEN:
        raise ValueError(f"library entries have 1 to {SEQ_MAX_LEN} slots, got Ld = {Ld}")
    scoring = _seq_scoring(mode, matrix, gap_open, gap_extend)
    a = _capi.SeqSearchArgs()
    dev = aa.device
    keep = [aa.to(dev, torch.int64).contiguous(), _bytes(mask, dev), db_aa.to(dev, torch.int64).contiguous(),
            db_len.to(dev, torch.int32).contiguous()]
    keep.append(scoring(a, dev))
    _bind_in(a, aa=keep[0], mask=keep[1])
    if D:
        _bind_in(a, db_aa=keep[2], db_len=keep[3])
    a.Q, a.N, a.D, a.Ld = Q, N, D, Ld
    out = {k: torch.empty(Q, dtype=torch.int32, device=dev) for k in ("best_index", "best_score", "best_n_ident", "best_n_columns")}
    out["best_identity"] = torch.empty(Q, dtype=torch.float64, device=dev)
    _bind_out(a, out)
    if Q:
        _capi.check(_capi.load().pf_seq_search_fwd(C.byref(a), _capi.stream_ptr()), "pf_seq_search_fwd")
    return out


def _mirrored_f64(B, pairs, dev, values, diag):
    """`_mirrored` for one float64 [P] result (the sequence ratios and identities are float64 quotients of integers)"""
    i, j = pairs[:, 0].to(dev, torch.int64), pairs[:, 1].to(dev, torch.int64)
    m = torch.full((B, B), float("nan"), dtype=torch.float64, device=dev)
    m[i, j] = values
    m[j, i] = values
    return m.masked_fill(torch.eye(B, dtype=torch.bool, device=dev), diag)


def pairwise_sequence_ratio(aa, mask, groups=None):
    """aa, mask [B,N] -> ratio [B,B] float64: `sequence_ratio` of every pair i < j of the same group (all one group when `groups` is
    None), mirrored, with a diagonal of 1; pairs across groups are NaN.  difflib's ratio depends on the direction (about a quarter
    of random short pairs over four letters differ): the one kept is a = sequence i, b = sequence j with i < j."""
    B = aa.shape[0]
    pairs = _within_groups(B, groups)
    return _mirrored_f64(B, pairs, aa.device, sequence_ratio(aa, aa, mask, mask, pairs)["ratio"], 1.0)


def pairwise_sequence_identity(aa, mask, groups=None, **align):
    """aa, mask [B,N] -> identity [B,B] float64: the `sequence_align` identity (n_ident / n_columns; **align: mode, matrix, gap_open,
    gap_extend) of every pair i < j of the same group, x = sequence i, y = sequence j, mirrored, with a diagonal of 1; pairs across
    groups are NaN (and so is a pair without an aligned column).  1 - this matrix is a `dist` that `cluster` takes."""
    B = aa.shape[0]
    pairs = _within_groups(B, groups)
    return _mirrored_f64(B, pairs, aa.device, sequence_align(aa, aa, mask, mask, pairs, **align)["identity"], 1.0)


CLUSTER_MAX_N = 1024        # PF_CLUSTER_MAX_N: the most samples one group may hold
CLUSTER_METHODS = ("gromos", "single", "complete", "average")      # pf_cluster_args.method 0..3


def cluster(dist, cutoff, groups=None, method="gromos", score=None):
    """pf_cluster_fwd: the samples of each group clustered on the distance matrix `dist` [B,B] (a device tensor; what the pairwise_*
    functions return: symmetric, NaN across groups), one launch, one workgroup per group, nothing read back and no synchronisation.

    groups [B]: any integer labels on the host, as `group_pairs` takes (None: one group), at most CLUSTER_MAX_N samples each.  A
    sample's position is its rank inside its group.  For positions a < b only dist[a, b] right of the diagonal is read; NaN counts as
    +inf and is never within `cutoff` (>= 0; +inf is taken as the largest float).
    method: "gromos" -- Daura et al. 1999: the active sample with the most active neighbours (d <= cutoff, itself included; of equal
    counts the smallest position) leaves with them as the next cluster, labels in that order, the representative is that centre;
    "single" / "complete" / "average" -- agglomerative: the pair of clusters with the smallest linkage distance (of equal distances
    the smallest (i, j), a cluster named by its smallest position) merges while that distance is <= cutoff, i.e. the dendrogram cut
    at height cutoff; labels by size descending, then smallest position; the representative is the medoid (smallest fp64 sum of
    distances to the other members, of equal sums the smallest position).
    The linkages are checked against scipy's fcluster(criterion="distance"), as partitions only; gromos follows the publication and
    is not checked against GROMACS.
    score [B] (optional, lower is better): adds `best`.

    -> dict of device tensors: label [B] int32 (the cluster number inside the own group, 0 first), cluster_size [B], representative
    [B] (a batch index), best [B] (with score: the batch index of the own cluster's member with the lowest score, NaN last, of equal
    scores the smallest position), n_neighbours [B] (samples of the group within cutoff, itself included; every method),
    n_clusters [G]; index [B], offsets [G+1] int32 (the batch indices sorted by group, and the groups' ranges in it),
    group_labels [G] (sorted), group_of [B] (an index into group_labels)."""
    if not isinstance(dist, torch.Tensor) or dist.dim() != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError(f"dist must be a [B,B] tensor, got {tuple(getattr(dist, 'shape', ()))}")
    B = dist.shape[0]
    if method not in CLUSTER_METHODS:
        raise ValueError(f"method must be one of {CLUSTER_METHODS}, got {method!r}")
    cutoff = float(cutoff)
    if not cutoff >= 0.0:
        raise ValueError(f"cutoff must be >= 0, got {cutoff}")
    if score is not None and (not isinstance(score, torch.Tensor) or tuple(score.shape) != (B,)):
        raise ValueError(f"score must be [B] = {(B,)}, got {tuple(getattr(score, 'shape', ()))}")
    g = torch.zeros(B, dtype=torch.int64) if groups is None else torch.as_tensor(groups).reshape(-1).cpu()
    if g.numel() != B:
        raise ValueError(f"groups has {g.numel()} labels for {B} samples")
    labels, inv, counts = torch.unique(g, sorted=True, return_inverse=True, return_counts=True)
    G, n_max = labels.numel(), int(counts.max()) if B else 0
    if n_max > CLUSTER_MAX_N:
        raise ValueError(f"at most {CLUSTER_MAX_N} samples per group, got {n_max}")
    a = _capi.ClusterArgs()
    dev = dist.device
    keep = [_f32(dist, dev), None if score is None else _f32(score, dev)]
    _bind_in(a, dist=keep[0], score=keep[1])
    offsets = torch.zeros(G + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    out = {k: torch.empty(B, dtype=torch.int32, device=dev) for k in ("label", "cluster_size", "representative", "n_neighbours")}
    if score is not None:
        out["best"] = torch.empty(B, dtype=torch.int32, device=dev)
    out["n_clusters"] = torch.empty(G, dtype=torch.int32, device=dev)
    _bind_out(a, out)
    out["index"] = torch.argsort(inv, stable=True).to(torch.int32).to(dev)
    out["offsets"] = offsets.to(torch.int32).to(dev)
    _bind_in(a, index=out["index"], offsets=out["offsets"])
    a.B, a.G, a.n_max, a.method, a.cutoff = B, G, n_max, CLUSTER_METHODS.index(method), cutoff
    if B:
        lib = _capi.load()
        work = G * lib.pf_cluster_work_bytes(n_max, a.method)
        if work:
            keep.append(torch.empty(work, dtype=torch.uint8, device=dev))
            a.work = keep[-1].data_ptr()
        _capi.check(lib.pf_cluster_fwd(C.byref(a), _capi.stream_ptr()), "pf_cluster_fwd")
    out["group_labels"], out["group_of"] = labels.to(dev), inv.to(dev)
    return out


DSSP_MAX_N = 512            # PF_DSSP_MAX_N: the longest chain slot pf_dssp_fwd takes
SS_SYMBOLS = "HBEGITS-"     # 8-state codes 0..7: SSTRUCT_SYMB_TO_INDEX of pepflow/modules/protein/dssp.py
SS_SIMPLE = "HEC"           # simplified codes 0..2 (mdtraj's compute_dssp(simplified=True))
SS_MASKED = 255


def dssp(pos, mask, chain=None, aa=None, hbonds=False):
    """pf_dssp_fwd: DSSP 8-state secondary structure of each row (DSSP 2.x conventions, listed in csrc/dssp.hip).

    pos [B,N,A,3] with atoms 0..3 = N, CA, C, O (pos_heavyatom is read as it is), A >= 4; mask [B,N] the residues taken part;
    chain [B,N] (optional: a change of id breaks the chain); aa [B,N] (optional, only to find prolines, which are no H-bond donors).
    N <= DSSP_MAX_N.
    -> ss [B,N] uint8 device tensor (codes of SS_SYMBOLS, 255 where mask is false); with `hbonds` also hb_acc [B,N,2] int32 (each
    donor's two lowest-energy acceptors below 0 kcal/mol, -1: none) and hb_energy [B,N,2] float32 (0 with -1): (ss, hb_acc,
    hb_energy).  A bond is an entry with energy < -0.5."""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 4 or pos.shape[3] != 3 or pos.shape[2] < 4:
        raise ValueError(f"pos must be [B,N,A,3] with A >= 4 (N, CA, C, O first), got {tuple(getattr(pos, 'shape', ()))}")
    B, N, A, _ = pos.shape
    if tuple(mask.shape) != (B, N):
        raise ValueError(f"mask must be [B,N] = {(B, N)}, got {tuple(mask.shape)}")
    for nm, t in (("chain", chain), ("aa", aa)):
        if t is not None and tuple(t.shape) != (B, N):
            raise ValueError(f"{nm} must be [B,N] = {(B, N)}, got {tuple(t.shape)}")
    if N > DSSP_MAX_N:
        raise ValueError(f"dssp: N = {N} residues exceeds the kernel's bound of {DSSP_MAX_N}")
    dev = pos.device
    keep = [_f32(pos, dev), _bytes(mask, dev)] + [None if t is None else t.to(dev, torch.int64).contiguous() for t in (chain, aa)]
    a = _capi.DsspArgs()
    _bind_in(a, pos=keep[0], mask=keep[1], chain=keep[2], aa=keep[3])
    ss = torch.empty(B, N, dtype=torch.uint8, device=dev)
    a.ss = ss.data_ptr()
    if hbonds:
        acc, en = torch.empty(B, N, 2, dtype=torch.int32, device=dev), torch.empty(B, N, 2, device=dev)
        a.hb_acc, a.hb_energy = acc.data_ptr(), en.data_ptr()
    a.B, a.N, a.n_atoms, a.pro = B, N, A, _proline()
    if B and N:
        _capi.check(_capi.load().pf_dssp_fwd(C.byref(a), _capi.stream_ptr()), "pf_dssp_fwd")
    return (ss, acc, en) if hbonds else ss


def _proline():
    from .preprocess import residue_type
    return residue_type("PRO")


def ss_simplify(ss):
    """8-state codes -> mdtraj's simplified ones: 0 'H' (H, G, I), 1 'E' (E, B), 2 'C' (T, S, '-'); 255 stays 255"""
    def make():             # H, G, I -> 0 'H'; E, B -> 1 'E'; T, S, '-' -> 2 'C'; anything else (255 masked) -> 255
        t = torch.full((256,), SS_MASKED, dtype=torch.uint8)
        t[:8] = torch.tensor([0, 1, 1, 0, 0, 2, 2, 2], dtype=torch.uint8)
        return t
    return _table("ss_simplify", ss.device, make)[ss.long()]


def ss_strings(ss, simplified=False):
    """ss [B,N] 8-state codes -> one string per row, a character per unmasked residue ("HBEGITS-", or "HEC" with `simplified`),
    masked residues left out: what joining mdtraj's per-residue codes of the sliced chain gives (with '-' for its ' ')."""
    if simplified:
        ss, sym = ss_simplify(ss), SS_SIMPLE
    else:
        sym = SS_SYMBOLS
    rows = ss.reshape(-1, ss.shape[-1]).cpu().tolist()
    return ["".join(sym[c] for c in row if c < len(sym)) for row in rows]


VDW_RADIUS = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}    # openfold/np/residue_constants.py van_der_waals_radius
VIOLATION_SLOTS = 14
_UNK_ELEMENTS = "NCCO"          # a residue type >= 20: N, CA, C, O only


def vdw_radius_table():
    """-> [21,14] float32 CPU tensor: the van der Waals radius of heavy-atom slot s of residue type t (the package's numbering),
    from the first letter of the slot's atom name in the package's own table (data/rigid_groups.npz); 0 where the type has no
    such atom.  Row 20 (any type outside 0..19) has N, CA, C, O."""
    from .preprocess import _tables
    names = _tables()["atom_names"]
    tab = torch.zeros(21, VIOLATION_SLOTS)
    for t in range(20):
        for s in range(VIOLATION_SLOTS):
            if names[t][s]:
                tab[t, s] = VDW_RADIUS[names[t][s][0]]
    for s, e in enumerate(_UNK_ELEMENTS):
        tab[20, s] = VDW_RADIUS[e]
    return tab


def structural_violations(pos, atom_mask, aa, residue_index, query=None, group=None, violation_tolerance_factor=12.0,
                          clash_overlap_tolerance=1.5):
    """pf_violations_fwd: AlphaFold's between-residue structural violations (Jumper et al. 2021, Suppl. 1.9.11) with the values of
    OpenFold's between_residue_clash_loss, between_residue_bond_loss and extreme_ca_ca_distance_violations (conventions:
    csrc/violations.hip).

    pos [B,N,A,3] heavy atoms in the package's order, A >= 14, slots 0..13 are read (pos_heavyatom passes as it is); atom_mask
    [B,N,A]; aa [B,N] residue types in the package's numbering; residue_index [B,N] integers: a peptide bond is tested between n
    and n + 1 where it grows by exactly 1, and residues of equal index are never compared for clashes; query [B,N] (optional): only
    atom pairs with an atom in a query residue are evaluated; group [B,N] (optional): adds the *_cross outputs, over partners of
    another group.
    -> dict of device tensors: clash_atom_loss [B,N,14] float32, clash_atom [B,N,14] bool, clash_atom_pairs [B,N,14] int32,
    clash_mean_loss [B]; with `group` clash_atom_loss_cross, clash_atom_cross; bond_c_n_loss_mean, angle_ca_c_n_loss_mean,
    angle_c_n_ca_loss_mean [B]; connection_loss [B,N]; connection_violation [B,N] bool; ca_ca_break [B,N] bool (connection
    (n, n + 1) at n); ca_ca_extreme [B]."""
    dev, (B, N, A), pos, atom_mask, (aa, residue_index, query, group) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int32), ("query", query, torch.uint8), ("group", group, torch.uint8)))
    a = _capi.ViolationsArgs()
    _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index, query=query, group=group)
    a.radius = _table("vdw_radius", dev, vdw_radius_table).data_ptr()
    S = VIOLATION_SLOTS
    f32 = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)  # noqa: E731
    out = {"clash_atom_loss": f32(B, N, S), "clash_atom": u8(B, N, S),
           "clash_atom_pairs": torch.empty(B, N, S, dtype=torch.int32, device=dev), "clash_mean_loss": f32(B)}
    if group is not None:
        out.update(clash_atom_loss_cross=f32(B, N, S), clash_atom_cross=u8(B, N, S))
    out.update(bond_c_n_loss_mean=f32(B), angle_ca_c_n_loss_mean=f32(B), angle_c_n_ca_loss_mean=f32(B), connection_loss=f32(B, N),
               connection_violation=u8(B, N), ca_ca_break=u8(B, N), ca_ca_extreme=f32(B))
    _bind_out(a, out)
    a.B, a.N, a.n_atoms, a.pro = B, N, A, _proline()
    a.violation_tolerance_factor, a.clash_overlap_tolerance = float(violation_tolerance_factor), float(clash_overlap_tolerance)
    if B and N:
        _capi.check(_capi.load().pf_violations_fwd(C.byref(a), _capi.stream_ptr()), "pf_violations_fwd")
    else:
        for v in out.values():
            v.zero_()
    _as_bool(out, "clash_atom", "clash_atom_cross", "connection_violation", "ca_ca_break")
    return out


SASA_SLOTS = 15
SASA_MAX_POINTS, SASA_MAX_N = 1024, 512


def sasa_radius_table():
    """-> [21,15] float32 CPU tensor: slots 0..13 are `vdw_radius_table`, slot 14 (OXT) is an oxygen in every row."""
    tab = torch.zeros(21, SASA_SLOTS)
    tab[:, :VIOLATION_SLOTS] = vdw_radius_table()
    tab[:, 14] = VDW_RADIUS["O"]
    return tab


def sphere_points(n_points):
    """-> [P,3] float32 CPU tensor: P points of a golden spiral on the unit sphere, computed in float64 and rounded:
    y = (2k + 1) / P - 1, r = sqrt(1 - y^2), phi = k pi (3 - sqrt 5), u_k = (r cos phi, y, r sin phi) for k = 0 .. P - 1."""
    if not isinstance(n_points, int) or isinstance(n_points, bool) or not 1 <= n_points <= SASA_MAX_POINTS:
        raise ValueError(f"n_points must be an integer in 1..{SASA_MAX_POINTS}, got {n_points!r}")
    k = torch.arange(n_points, dtype=torch.float64)
    y = (2.0 * k + 1.0) / n_points - 1.0
    r = torch.sqrt(1.0 - y * y)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return torch.stack([r * torch.cos(phi), y, r * torch.sin(phi)], 1).to(torch.float32)


def sasa(pos, atom_mask, aa, query=None, group=None, probe_radius=1.4, n_points=960):
    """pf_sasa_fwd: Shrake-Rupley solvent-accessible surface area of heavy-atom structures (conventions: csrc/sasa.hip).  Bondi
    radii (`sasa_radius_table`), a probe of 1.4 A and 960 points are also mdtraj's shrake_rupley defaults; there are no hydrogens.

    pos [B,N,A,3] heavy atoms in the package's order, A >= 14, slots 0 .. min(A,15)-1 are read (pos_heavyatom passes as it is);
    atom_mask [B,N,A]; aa [B,N] residue types in the package's numbering; N <= 512.  query [B,N] (optional): only atoms of query
    residues are evaluated, every existing atom is still a partner; the others get count -1 and area 0.  group [B,N] bool
    (optional): adds the *_own outputs, the same quantities with only atoms of residues of the own group as partners -- every group
    on its own, so sasa_*_own - sasa_* is the area buried by the other group.
    -> dict of device tensors: count [B,N,15] int32 accessible points, sasa_atom [B,N,15] float32 = 4 pi (radius + probe)^2 count /
    n_points, sasa_residue [B,N], sasa_total [B]; with `group` count_own, sasa_atom_own, sasa_residue_own, sasa_total_own."""
    points = sphere_points(n_points)                # checks n_points
    probe_radius = float(probe_radius)
    if not 0.0 <= probe_radius < 1e6:
        raise ValueError(f"probe_radius must be >= 0, got {probe_radius}")
    dev, (B, N, A), pos, atom_mask, (aa, query, group) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("query", query, torch.uint8), ("group", group, torch.uint8)), max_n=SASA_MAX_N)
    a = _capi.SasaArgs()
    _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, query=query, group=group)
    a.radius = _table("sasa_radius", dev, sasa_radius_table).data_ptr()
    a.points = _table("sphere_points", dev, lambda: points, n_points).data_ptr()
    S = SASA_SLOTS
    f32 = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"count": i32(B, N, S), "sasa_atom": f32(B, N, S), "sasa_residue": f32(B, N), "sasa_total": f32(B)}
    if group is not None:
        out.update(count_own=i32(B, N, S), sasa_atom_own=f32(B, N, S), sasa_residue_own=f32(B, N), sasa_total_own=f32(B))
    _bind_out(a, out)
    a.B, a.N, a.n_atoms, a.n_points, a.probe_radius = B, N, A, n_points, probe_radius
    if B and N:
        work = f32(B, N, 4)                         # the residue-sized workspace: centre and padded extent
        a.work = work.data_ptr()
        _capi.check(_capi.load().pf_sasa_fwd(C.byref(a), _capi.stream_ptr()), "pf_sasa_fwd")
    else:
        for v in out.values():
            v.zero_()
    return out


CAVITY_MAX_N, CAVITY_MAX_POINTS, CAVITY_MAX_OUT = 4096, 128 ** 3, 32
CAVITY_DEFAULTS = {"probe": 1.4, "max_ray": 12.0, "min_buried": 5, "connectivity": 6, "min_points": 8, "max_cavities": 8,
                   "r_lining": 4.5}
CAVITY_STATUS = {1: "a path to a root", 2: "the retries of a link", 4: "the list of components"}


def cavity_grid(pos, atom_mask, h=1.0, margin=8.0):
    """The grid of `cavity_scan` around structures: the bounding box of the atoms of pos [B,N,A,3] with atom_mask [B,N,A] set, padded
    by `margin` on every side, its lower corner snapped down to a multiple of h.  A host computation (float64, the tensors are read
    back).  -> (origin [B,3] float32 CPU tensor, (nx, ny, nz)): the dimensions are those of the largest structure; a structure without
    atoms gets the origin 0."""
    h, margin = float(h), float(margin)
    if not (h > 0.0 and math.isfinite(h)) or not (margin >= 0.0 and math.isfinite(margin)):
        raise ValueError(f"h must be > 0 and margin >= 0, got {h}, {margin}")
    if pos.dim() != 4 or pos.shape[3] != 3 or tuple(atom_mask.shape) != tuple(pos.shape[:3]):
        raise ValueError(f"pos must be [B,N,A,3] and atom_mask [B,N,A], got {tuple(pos.shape)}, {tuple(atom_mask.shape)}")
    B = pos.shape[0]
    p, m = pos.detach().cpu().double().reshape(B, -1, 3), atom_mask.detach().cpu().bool().reshape(B, -1)
    origin, dims = torch.zeros(B, 3, dtype=torch.float64), [1, 1, 1]
    for b in range(B):
        if not m[b].any():
            continue
        x = p[b][m[b]]
        lo = torch.floor((x.min(0).values - margin) / h)
        hi = torch.ceil((x.max(0).values + margin) / h)
        origin[b] = lo * h
        dims = [max(d, int(n)) for d, n in zip(dims, (hi - lo + 1).tolist())]
    return origin.to(torch.float32), tuple(dims)


def _cavity_params(h, params):
    """the scan's parameters, checked (ValueError) -> (dict with the defaults filled in, n_axis, n_diag)"""
    unknown = set(params) - set(CAVITY_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown cavity scan parameters {sorted(unknown)}; known: {sorted(CAVITY_DEFAULTS)}")
    p = {**CAVITY_DEFAULTS, **params}
    if not (h > 0.0 and h < 1e6):
        raise ValueError(f"h must be > 0, got {h}")
    for k in ("probe", "max_ray", "r_lining"):
        p[k] = float(p[k])
        if not 0.0 <= p[k] < 1e6:
            raise ValueError(f"{k} must be >= 0, got {p[k]}")
    for k in ("min_buried", "connectivity", "min_points", "max_cavities"):
        if not isinstance(p[k], int) or isinstance(p[k], bool):
            raise ValueError(f"{k} must be an integer, got {p[k]!r}")
    if not 1 <= p["min_buried"] <= 7:
        raise ValueError(f"min_buried must be in 1..7, got {p['min_buried']}")
    if p["connectivity"] not in (6, 26):
        raise ValueError(f"connectivity must be 6 or 26, got {p['connectivity']}")
    if p["min_points"] < 1 or not 1 <= p["max_cavities"] <= CAVITY_MAX_OUT:
        raise ValueError(f"min_points must be >= 1 and max_cavities in 1..{CAVITY_MAX_OUT}, got {p['min_points']}, {p['max_cavities']}")
    return p, int(math.floor(p["max_ray"] / h)), int(math.floor(p["max_ray"] / (h * math.sqrt(3.0))))


def cavity_scan(pos, atom_mask, aa, origin, dims, h=1.0, radius=None, check=True, **params):
    """pf_cavity_fwd: a LIGSITE-style buriedness scan (Hendlich et al. 1997) over a grid around heavy-atom structures, the connected
    cavities of the buried free points, their ranking and lining residues; the definitions are in include/pepflow_hip.h and
    csrc/cavity.hip, tests/cavity_oracle.py restates them.  Not checked against the LIGSITE program or fpocket; defaults untuned.

    pos [B,N,A,3] heavy atoms in the package's order (A >= 14, slots 0 .. min(A,15)-1 are read), atom_mask [B,N,A], aa [B,N], all on
    the device; N <= 4096.  origin [B,3] and dims = (nx, ny, nz) (`cavity_grid`), nx * ny * nz <= 128^3, spacing h; point (ix, iy, iz)
    has the linear index (ix * ny + iy) * nz + iz and lies at origin + index * h.  radius [21,15] (default `sasa_radius_table`).
    params: CAVITY_DEFAULTS (probe, max_ray, min_buried, connectivity, min_points, max_cavities = K, r_lining).
    -> dict of device tensors: occupied [B,G] bool, buried [B,G] uint8 (0..7, 255 where occupied), label [B,G] int32 (rank or -1),
    n_found [B] int32, size [B,K] int32, center [B,K,3], mean_buried [B,K], lining [B,K,N] bool, status [1] int32.
    `check` reads the status word back and raises PepflowHipError when a device loop ran out of its bound; it is skipped while the
    stream is being captured (the call makes no host read then: check out["status"] after a replay)."""
    h = float(h)
    p, n_axis, n_diag = _cavity_params(h, params)
    try:
        nx, ny, nz = (int(d) for d in dims)
    except (TypeError, ValueError):
        raise ValueError(f"dims must be three integers, got {dims!r}") from None
    if min(nx, ny, nz) < 1 or nx * ny * nz > CAVITY_MAX_POINTS:
        raise ValueError(f"dims must be >= 1 with at most {CAVITY_MAX_POINTS} points in all, got {(nx, ny, nz)}")
    dev, (B, N, A), pos, atom_mask, (aa,) = _structure(pos, atom_mask, (("aa", aa, torch.int64),), max_n=CAVITY_MAX_N)
    if not isinstance(origin, torch.Tensor) or tuple(origin.shape) != (B, 3):
        raise ValueError(f"origin must be a [B,3] = {(B, 3)} tensor, got {tuple(getattr(origin, 'shape', ()))}")
    if radius is not None and tuple(radius.shape) != (21, SASA_SLOTS):
        raise ValueError(f"radius must be [21,{SASA_SLOTS}], got {tuple(radius.shape)}")
    if B > 65535:
        raise ValueError(f"at most 65535 structures per call, got {B}")
    origin = _f32(origin, dev)
    radius = _table("sasa_radius", dev, sasa_radius_table) if radius is None else _f32(radius, dev)
    a = _capi.CavityArgs()
    _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, radius=radius, origin=origin)
    G, K = nx * ny * nz, p["max_cavities"]
    new = lambda dt, *shape: torch.empty(*shape, dtype=dt, device=dev)  # noqa: E731
    out = {"occupied": new(torch.uint8, B, G), "buried": new(torch.uint8, B, G), "label": new(torch.int32, B, G),
           "n_found": new(torch.int32, B), "size": new(torch.int32, B, K), "center": new(torch.float32, B, K, 3),
           "mean_buried": new(torch.float32, B, K), "lining": new(torch.uint8, B, K, N),
           "status": torch.zeros(1, dtype=torch.int32, device=dev)}
    _bind_out(a, out)
    a.B, a.N, a.n_atoms, a.nx, a.ny, a.nz, a.n_axis, a.n_diag = B, N, A, nx, ny, nz, n_axis, n_diag
    a.min_buried, a.connectivity, a.min_points, a.max_cavities = p["min_buried"], p["connectivity"], p["min_points"], K
    a.h, a.probe, a.r_lining = h, p["probe"], p["r_lining"]
    if B:
        lib = _capi.load()
        work = new(torch.uint8, B * lib.pf_cavity_work_bytes(nx, ny, nz))
        a.work = work.data_ptr()
        _capi.check(lib.pf_cavity_fwd(C.byref(a), _capi.stream_ptr()), "pf_cavity_fwd")
        if N == 0:
            out["lining"].zero_()
        if check and not torch.cuda.is_current_stream_capturing():
            cavity_check(out["status"])
    _as_bool(out, "occupied", "lining")
    return out


def cavity_check(status):
    """raises PepflowHipError when `cavity_scan`'s status word says that a device loop ran out of its bound (a host read)"""
    s = int(status.item())
    if s:
        what = ", ".join(v for k, v in CAVITY_STATUS.items() if s & k)
        raise _capi.PepflowHipError(f"pf_cavity_fwd: a device loop exhausted its bound ({what}; status {s}); the outputs are not valid")


TORSION_NAMES = ("omega", "phi", "psi", "psi_o", "chi1", "chi2", "chi3", "chi4")
# Stated from chemistry, resolved against the package's own atom-name table: the chi angles whose two end atoms are equivalent (the
# angle is defined up to pi), and the atom pairs that a 180 degree flip of that chi exchanges.
PI_PERIODIC_CHI = {"ASP": 2, "GLU": 3, "PHE": 2, "TYR": 2}
EQUIVALENT_ATOMS = {"ASP": (("OD1", "OD2"),), "GLU": (("OE1", "OE2"),), "PHE": (("CD1", "CD2"), ("CE1", "CE2")),
                    "TYR": (("CD1", "CD2"), ("CE1", "CE2"))}


def chi_atom_table():
    """-> [21,4,4] int32 CPU tensor: the heavy-atom slots of chi1-4 of each residue type (data/chi_atoms.npz), -1: no such angle"""
    from .preprocess import _tables
    return _tables()["chi_atom_idx"][:21].to(torch.int32).contiguous()


def pi_periodic_table():
    """-> [21,4] bool CPU tensor: chi k + 1 of type t is pi-periodic (PI_PERIODIC_CHI by residue name)"""
    from .preprocess import _tables
    tab = torch.zeros(21, 4, dtype=torch.bool)
    for name, chi in PI_PERIODIC_CHI.items():
        tab[_tables()["res_index"][name], chi - 1] = True
    return tab


def swap_table():
    """-> [21,4] uint8 CPU tensor: (a1, b1, a2, b2), the slots of up to two pairs of equivalent atoms of type t (EQUIVALENT_ATOMS by
    residue and atom name); (0, 0) where unused"""
    from .preprocess import _tables
    t = _tables()
    tab = torch.zeros(21, 4, dtype=torch.uint8)
    for name, pairs in EQUIVALENT_ATOMS.items():
        r = t["res_index"][name]
        for k, (u, v) in enumerate(pairs):
            tab[r, 2 * k], tab[r, 2 * k + 1] = t["atom_names"][r].index(u), t["atom_names"][r].index(v)
    return tab


def torsion_angles(pos, atom_mask, aa, residue_index=None):
    """pf_torsions_fwd: the torsion angles of heavy-atom structures (conventions: csrc/torsions.hip).

    pos [B,N,A,3] heavy atoms in the package's order, A >= 14, slots 0..13 are read (pos_heavyatom passes as it is); atom_mask
    [B,N,A]; aa [B,N] residue types in the package's numbering; residue_index [B,N] (optional, metrics.residue_index): residues are
    bonded where it grows by exactly 1; None: consecutive positions are bonded.
    -> dict of device tensors: angles [B,N,8] float32 in [0, 2 pi), slots TORSION_NAMES: omega (CA(n-1), C(n-1), N, CA), phi, psi,
    psi_o (N, CA, C, O: slot 0 of preprocess.get_torsion_angle; on coordinates rebuilt by full_atom it is the model's first angle
    + pi), chi1..chi4; defined [B,N,8] bool: all four atoms in atom_mask, the neighbour bonded (backbone angles), the type has the chi,
    no degenerate geometry.  Undefined angles are 0, never NaN."""
    dev, (B, N, A), pos, atom_mask, (aa, residue_index) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int32)))
    a = _capi.TorsionsArgs()
    _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index)
    a.chi_atoms = _table("chi_atoms", dev, chi_atom_table).data_ptr()
    out = {"angles": torch.empty(B, N, 8, device=dev), "defined": torch.empty(B, N, 8, dtype=torch.uint8, device=dev)}
    _bind_out(a, out)
    a.B, a.N, a.n_atoms = B, N, A
    if B and N:
        _capi.check(_capi.load().pf_torsions_fwd(C.byref(a), _capi.stream_ptr()), "pf_torsions_fwd")
    _as_bool(out, "defined")
    return out


_COMPARE_KEYS = ("pos", "atom_mask", "aa", "angles", "defined")


def sidechain_compare(x, y, pairs, correct_tol=math.radians(20), per_residue=False):
    """pf_sidechain_compare_fwd over the work list `pairs` [P,2] (pair p = (i, j): x[i] against y[j], residue by residue).

    x, y: dicts with pos [B.,N,A.,3], atom_mask [B.,N,A.], aa [B.,N] and the angles / defined [B.,N,8] of `torsion_angles` (y may be
    x).  correct_tol: radians.
    -> dict of device tensors.  Per pair and angle slot [P,8]: err_sum float64 (radians), err_count, within int32 -- over the residues
    where both angles are defined (slots 3..7: and the types are equal and in 0..19), the absolute difference wrapped to [0, pi], to
    [0, pi/2] for the pi-periodic chi (PI_PERIODIC_CHI); within counts errors <= correct_tol.  Per pair [P]: res_with_chi (residues
    with a compared chi), res_correct (those with every compared chi within correct_tol), sc_sq_sum float64, sc_atoms int32, sc_rmsd
    float32 (NaN without atoms): side-chain slots 4..13 of residues of equal type, each in its own backbone frame, the smaller of the
    sum as it is and with EQUIVALENT_ATOMS exchanged.  With `per_residue`: err [P,N,8] (NaN where not compared), sc_sq [P,N], sc_n
    [P,N] int32, swapped [P,N] bool."""
    for nm, d in (("x", x), ("y", y)):
        if not isinstance(d, dict) or any(k not in d for k in _COMPARE_KEYS):
            raise ValueError(f"{nm} must be a dict with {_COMPARE_KEYS}")
    pairs = _check_pairs(pairs)
    correct_tol = float(correct_tol)
    if not 0.0 <= correct_tol <= math.pi:
        raise ValueError(f"correct_tol must be in [0, pi] radians, got {correct_tol}")
    dev = x["pos"].device

    def aligned(t, n):      # the kernel reads angles as float4 and defined 8 bytes at a time: a view at an odd offset is copied
        return t if t.data_ptr() % n == 0 else t.clone()

    def side(d, nm):
        _, (B, N, A), pos, atom_mask, (aa,) = _structure(d["pos"], d["atom_mask"], (("aa", d["aa"], torch.int64),), tag=nm + ".", dev=dev)
        for k in ("angles", "defined"):
            if tuple(d[k].shape) != (B, N, 8):
                raise ValueError(f"{nm}.{k} must be {(B, N, 8)}, got {tuple(d[k].shape)}")
        return (B, N, A), dict(pos=pos, mask=atom_mask, aa=aa, angles=aligned(_f32(d["angles"], dev), 16),
                               defined=aligned(_bytes(d["defined"], dev), 8))
    (Bx, N, Ax), kx = side(x, "x")
    (By, Ny, Ay), ky = ((Bx, N, Ax), kx) if y is x else side(y, "y")
    if Ny != N:
        raise ValueError(f"x and y must have the same number of residues, got {N} and {Ny}")
    if N == 0 or Bx == 0 or By == 0:
        raise ValueError("sidechain_compare needs at least one structure of at least one residue on each side")
    pairs = pairs.to(dev, torch.int32).contiguous()
    P = pairs.shape[0]
    a = _capi.SidechainCompareArgs()
    _bind_in(a, pairs=pairs, **{f"{k}_x": t for k, t in kx.items()}, **{f"{k}_y": t for k, t in ky.items()})
    a.periodic = _table("pi_periodic", dev, lambda: pi_periodic_table().to(torch.uint8)).data_ptr()
    a.swap = _table("swap", dev, swap_table).data_ptr()
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"err_sum": torch.empty(P, 8, dtype=torch.float64, device=dev), "err_count": i32(P, 8), "within": i32(P, 8),
           "res_with_chi": i32(P), "res_correct": i32(P), "sc_sq_sum": torch.empty(P, dtype=torch.float64, device=dev),
           "sc_atoms": i32(P), "sc_rmsd": torch.empty(P, device=dev)}
    if per_residue:
        out.update(err=torch.empty(P, N, 8, device=dev), sc_sq=torch.empty(P, N, device=dev), sc_n=i32(P, N),
                   swapped=torch.empty(P, N, dtype=torch.uint8, device=dev))
    _bind_out(a, out)
    a.Bx, a.By, a.N, a.P, a.n_atoms_x, a.n_atoms_y, a.correct_tol = Bx, By, N, P, Ax, Ay, correct_tol
    if P:
        _capi.check(_capi.load().pf_sidechain_compare_fwd(C.byref(a), _capi.stream_ptr()), "pf_sidechain_compare_fwd")
    _as_bool(out, "swapped")
    return out


LDDT_MAX_N = 512            # PF_LDDT_MAX_N / PF_CONTACTS_MAX_N: the most residues pf_lddt_fwd and pf_contacts_fwd take
LDDT_SLOTS = 14             # PF_LDDT_SLOTS: the per-atom outputs of pf_lddt_fwd
SLOT_MASKS = {"ca": 0x2, "backbone": 0xF, "all": 0x3FFF}       # bit s: heavy-atom slot s (N, CA, C, O, then the side chain)


def _slot_mask(slots):
    if isinstance(slots, str) and slots in SLOT_MASKS:
        return SLOT_MASKS[slots]
    if isinstance(slots, int) and not isinstance(slots, bool) and 0 < slots < 1 << 15:
        return slots
    raise ValueError(f"slots must be one of {tuple(SLOT_MASKS)} or a bit mask of the slots 0..14, got {slots!r}")


def _positive(name, v):
    v = float(v)
    if not 0.0 < v < 1e6:
        raise ValueError(f"{name} must be a positive length in A, got {v}")
    return v


def _structure_pairs(a, name, x, y, pairs, group, query=None, with_aa=True):
    """The inputs of pf_lddt_fwd / pf_contacts_fwd: x, y dicts with pos [B.,N,A.,3], atom_mask [B.,N,A.], aa [B.,N] (y may be x), the
    work list pairs [P,2], group / query [By,N] (they belong to y); N <= LDDT_MAX_N.  Checks (ValueError), converts through
    `_structure` and binds everything into `a`.  -> (the tensors to keep alive, device, N, P)"""
    for nm, d in (("x", x), ("y", y)):
        if not isinstance(d, dict) or any(k not in d for k in _COMPARE_KEYS[:3]):
            raise ValueError(f"{nm} must be a dict with {_COMPARE_KEYS[:3]}")
    pairs = _check_pairs(pairs)
    dev = x["pos"].device if isinstance(x["pos"], torch.Tensor) else None

    def side(d, nm, extra=()):
        _, (B, N, A), pos, atom_mask, conv = _structure(d["pos"], d["atom_mask"], (("aa", d["aa"], torch.int64),) + extra,
                                                        max_n=LDDT_MAX_N, tag=nm + ".", dev=dev)
        return (B, N, A), [pos, atom_mask] + conv
    per_y = (("group", group, torch.uint8), ("query", query, torch.uint8))
    (By, Ny, Ay), ky = side(y, "y", per_y)
    (Bx, N, Ax), kx = ((By, Ny, Ay), ky) if y is x else side(x, "x")
    if Ny != N:
        raise ValueError(f"x and y must have the same number of residues, got {N} and {Ny}")
    if N == 0 or Bx == 0 or By == 0:
        raise ValueError(f"{name} needs at least one structure of at least one residue on each side")
    keep = kx[:3] + ky + [pairs.to(dev, torch.int32).contiguous()]
    _bind_in(a, pos_x=kx[0], mask_x=kx[1], pos_y=ky[0], mask_y=ky[1], group=ky[3], query=ky[4], pairs=keep[-1],
             **(dict(aa_x=kx[2], aa_y=ky[2]) if with_aa else {}))
    a.Bx, a.By, a.N, a.P, a.n_atoms_x, a.n_atoms_y = Bx, By, N, pairs.shape[0], Ax, Ay
    return keep, dev, N, pairs.shape[0]


def lddt(x, y, pairs, slots="all", cutoff=15.0, exclude_same_residue=False, group=None, query=None, per_atom=False):
    """pf_lddt_fwd over the work list `pairs` [P,2] (pair p = (i, j): the model x[i] against the reference structure y[j]): the local
    distance difference test with the values of OpenFold's `lddt` / `lddt_ca` (openfold/utils/loss.py:382-458; conventions:
    csrc/lddt.hip).  No superposition is involved.

    x, y: dicts with pos [B.,N,A.,3], atom_mask [B.,N,A.], aa [B.,N] as `sidechain_compare` takes them (y may be x); N <= 512.
    slots: "ca", "backbone" (N, CA, C, O), "all" (the 14 heavy-atom slots) or a bit mask of slots; an atom is compared where both masks
    have it and, for side-chain slots, the residue types agree.  A pair of compared atoms is scored when it is closer than `cutoff` in
    y; exclude_same_residue=False scores pairs inside a residue too, as the reference does (True: Mariani et al.'s lDDT).  group
    [By,N] (optional): adds the *_cross outputs, over partners of another group byte; query [By,N] (optional): only rows in query
    residues are evaluated, every compared atom is still a partner.
    -> dict of device tensors: scored, kept [P,N] int32 (per row residue: scored pairs, and the thresholds 0.5 / 1 / 2 / 4 A they
    keep); lddt_residue [P,N] = kept / (4 scored), lddt [P] from the counts summed over the rows, float64; with `group`
    scored_cross, kept_cross, lddt_residue_cross, lddt_cross; with `per_atom` scored_atom, kept_atom [P,N,14] (and *_atom_cross).
    Deviation from the reference: its (eps + sum) / (eps + n) gives 1.0 for a row without a scored pair; here such a row is NaN."""
    slot_mask, cutoff = _slot_mask(slots) & 0x3FFF, _positive("cutoff", cutoff)
    a = _capi.LddtArgs()
    keep, dev, N, P = _structure_pairs(a, "lddt", x, y, pairs, group, query)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"scored": i32(P, N), "kept": i32(P, N)}
    tags = ("", "_cross") if group is not None else ("",)
    if group is not None:
        out.update(scored_cross=i32(P, N), kept_cross=i32(P, N))
    if per_atom:
        for t in tags:
            out.update({"scored_atom" + t: i32(P, N, LDDT_SLOTS), "kept_atom" + t: i32(P, N, LDDT_SLOTS)})
    _bind_out(a, out)
    a.slot_mask, a.exclude_same_residue, a.cutoff = slot_mask, int(bool(exclude_same_residue)), cutoff
    if P:
        _capi.check(_capi.load().pf_lddt_fwd(C.byref(a), _capi.stream_ptr()), "pf_lddt_fwd")
    for t in tags:
        s, k = out["scored" + t].double(), out["kept" + t].double()
        out["lddt_residue" + t] = k / (4.0 * s)                 # 0 / 0: NaN where nothing is scored
        out["lddt" + t] = k.sum(1) / (4.0 * s.sum(1))
    return out


def interface_contacts(x, y, pairs, group, slots="all", contact_cutoff=5.0, interface_cutoff=10.0):
    """pf_contacts_fwd over the work list `pairs` [P,2]: the residue contacts between the groups in the model x[i] and in the reference
    structure y[j] at once (conventions: csrc/contacts.hip).  x, y as in `lddt`; group [By,N] (required) belongs to y.  A residue pair
    counts when its group bytes differ and both residues have an atom in both structures -- each structure on its own atom_mask, no
    residue-type rule; its distance is the smallest one between their atoms (slots: as in `lddt`; a mask may name slot 14, OXT).
    -> dict of device tensors, per row residue [P,N]: contacts_x, contacts_y, contacts_shared int32 (the partners within
    contact_cutoff in x, in y, in both); interface_x, interface_y bool (a partner within interface_cutoff); min_dist_x, min_dist_y
    float32 (the nearest atom of a counted partner, +inf without any).  Each residue pair shows in both of its rows."""
    if group is None:
        raise ValueError("interface_contacts needs `group` [By,N]: the contacts are those between residues of different groups")
    slot_mask = _slot_mask(slots)
    contact_cutoff, interface_cutoff = _positive("contact_cutoff", contact_cutoff), _positive("interface_cutoff", interface_cutoff)
    a = _capi.ContactsArgs()
    keep, dev, N, P = _structure_pairs(a, "interface_contacts", x, y, pairs, group, with_aa=False)
    out = {k: torch.empty(P, N, dtype=torch.int32, device=dev) for k in ("contacts_x", "contacts_y", "contacts_shared")}
    out.update({k: torch.empty(P, N, dtype=torch.uint8, device=dev) for k in ("interface_x", "interface_y")})
    out.update({k: torch.empty(P, N, device=dev) for k in ("min_dist_x", "min_dist_y")})
    _bind_out(a, out)
    a.slot_mask, a.contact_cutoff, a.interface_cutoff = slot_mask, contact_cutoff, interface_cutoff
    if P:
        _capi.check(_capi.load().pf_contacts_fwd(C.byref(a), _capi.stream_ptr()), "pf_contacts_fwd")
    _as_bool(out, "interface_x", "interface_y")
    return out


DOCKQ_CLASSES = ("incorrect", "acceptable", "medium", "high")       # dockq_class 0..3: DockQ < 0.23, < 0.49, < 0.80, >= 0.80


def dockq_score(fnat, irmsd, lrmsd):
    """DockQ = (Fnat + 1 / (1 + (iRMSD / 1.5)^2) + 1 / (1 + (LRMSD / 8.5)^2)) / 3 (Basu & Wallner, PLoS ONE 2016, eq. 1-2)"""
    return (fnat + 1.0 / (1.0 + (irmsd / 1.5) ** 2) + 1.0 / (1.0 + (lrmsd / 8.5) ** 2)) / 3.0


def dockq(x, y, pairs, group, contact_cutoff=5.0, interface_cutoff=10.0):
    """DockQ of the model x[i] against the native y[j] for every pair of `pairs` [P,2], written from the publication (Basu & Wallner,
    PLoS ONE 2016); it has not been checked against the DockQ program.  x, y as in `lddt`; group [By,N] belongs to y, != 0 marks the
    ligand (the peptide), 0 the receptor.  The CAPRI-peptide cut-offs are contact_cutoff=4.0, interface_cutoff=8.0.
    -> dict of device tensors, per pair [P], float64:
      fnat      the native's residue contacts (heavy atoms within contact_cutoff across the groups) that the model has: sum over the
                ligand of contacts_shared / contacts_y (NaN without native contacts);
      fnonnat   the model's contacts that the native lacks, over the model's (NaN without any);
      irmsd     `superpose`'s rmsd over N, CA, C, O of the native's interface residues (a partner within interface_cutoff in y; both
                sides of the interface) where both structures have the atom;
      lrmsd     the ligand's N, CA, C, O rmsd_plain after superposing the receptor's N, CA, C, O;
      dockq     `dockq_score`; dockq_class int64 0..3 (DOCKQ_CLASSES; 0 where dockq is NaN);
    n_native_contacts, n_sample_contacts, n_shared_contacts [P] int64 (summed over the ligand), n_interface [P] int64, and the
    outputs of `interface_contacts`.  A pair with an index out of range is NaN."""
    c = interface_contacts(x, y, pairs, group, "all", contact_cutoff, interface_cutoff)
    dev = c["contacts_x"].device
    pairs = _check_pairs(pairs).to(dev, torch.int64)
    Bx, N = x["pos"].shape[:2]
    By = y["pos"].shape[0]
    ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < Bx) & (pairs[:, 1] >= 0) & (pairs[:, 1] < By)
    i, j = pairs[:, 0].clamp(0, Bx - 1), pairs[:, 1].clamp(0, By - 1)
    lig = (torch.as_tensor(group).to(dev) != 0)[j] & ok[:, None]                       # [P,N]
    over = lambda t: (t.to(torch.int64) * lig).sum(1)  # noqa: E731
    n_y, n_x, n_s = over(c["contacts_y"]), over(c["contacts_x"]), over(c["contacts_shared"])
    fnat = n_s.double() / n_y.double()
    fnonnat = (n_x - n_s).double() / n_x.double()
    # the backbone atoms of each pair as one point set [P, 4 N, 3]; three masks on it
    P = pairs.shape[0]
    bx, by = _f32(x["pos"].to(dev)[i][:, :, :4], dev).reshape(P, 4 * N, 3), _f32(y["pos"].to(dev)[j][:, :, :4], dev).reshape(P, 4 * N, 3)
    both = (x["atom_mask"].to(dev)[i][:, :, :4] != 0) & (y["atom_mask"].to(dev)[j][:, :, :4] != 0) & ok[:, None, None]
    on = lambda m: (both & m[:, :, None]).reshape(P, 4 * N)  # noqa: E731
    diag = torch.arange(P, dtype=torch.int32, device=dev)[:, None].expand(P, 2)
    face, rec = on(c["interface_y"]), on(~lig & ok[:, None])
    irmsd = superpose(bx, by, face, face, diag)["rmsd"].double()
    placed = superpose(bx, by, rec, rec, diag, aligned=True)["aligned"]
    lrmsd = superpose(placed, by, on(lig), on(lig), diag)["rmsd_plain"].double()
    score = dockq_score(fnat, irmsd, lrmsd)
    cls = (score >= 0.23).long() + (score >= 0.49).long() + (score >= 0.80).long()
    res = {"fnat": fnat, "fnonnat": fnonnat, "irmsd": irmsd, "lrmsd": lrmsd, "dockq": score, "dockq_class": cls,
           "n_native_contacts": n_y, "n_sample_contacts": n_x, "n_shared_contacts": n_s, "n_interface": c["interface_y"].sum(1)}
    res.update(c)
    return res


# ---- empirical interface energy ----------------------------------------------------------------------------------------------------
# The functional form of AutoDock Vina's scoring function (Trott & Olson, J. Comput. Chem. 31, 2010) over heavy atoms.  Written from
# the publication and checked against a float64 restatement (tests/energy_oracle.py) and hand-computed cases; NOT checked against
# the Vina program, and neither Vina's output (no ligand preparation, no torsion tree, no hydrogens) nor Rosetta's dG_separated.
ENERGY_MAX_N = 512          # PF_INTERFACE_ENERGY_MAX_N
ENERGY_SLOTS = 15           # PF_INTERFACE_ENERGY_SLOTS
ENERGY_TERMS = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
VINA_WEIGHTS = (-0.0356, -0.00516, 0.840, -0.0351, -0.587)
XS_RADIUS = {"C": 1.9, "N": 1.8, "O": 1.7, "S": 2.0}
TYPE_HYDROPHOBIC, TYPE_DONOR, TYPE_ACCEPTOR = 1, 2, 4       # the bits of interface_type_table
# Stated from chemistry, resolved against the package's own atom-name table.  The covalent bonds of each side chain (CA-CB and
# beyond; proline's ring closes on N); the backbone's N-CA, CA-C, C-O, C-OXT and the peptide bond C-N are added for every type.
SIDE_CHAIN_BONDS = {
    "ALA": "CA-CB", "GLY": "",
    "CYS": "CA-CB CB-SG", "SER": "CA-CB CB-OG", "THR": "CA-CB CB-OG1 CB-CG2", "VAL": "CA-CB CB-CG1 CB-CG2",
    "ASP": "CA-CB CB-CG CG-OD1 CG-OD2", "ASN": "CA-CB CB-CG CG-OD1 CG-ND2",
    "GLU": "CA-CB CB-CG CG-CD CD-OE1 CD-OE2", "GLN": "CA-CB CB-CG CG-CD CD-OE1 CD-NE2",
    "ILE": "CA-CB CB-CG1 CB-CG2 CG1-CD1", "LEU": "CA-CB CB-CG CG-CD1 CG-CD2", "MET": "CA-CB CB-CG CG-SD SD-CE",
    "LYS": "CA-CB CB-CG CG-CD CD-CE CE-NZ", "ARG": "CA-CB CB-CG CG-CD CD-NE NE-CZ CZ-NH1 CZ-NH2", "PRO": "CA-CB CB-CG CG-CD CD-N",
    "HIS": "CA-CB CB-CG CG-ND1 CG-CD2 ND1-CE1 CD2-NE2 CE1-NE2",
    "PHE": "CA-CB CB-CG CG-CD1 CG-CD2 CD1-CE1 CD2-CE2 CE1-CZ CE2-CZ",
    "TYR": "CA-CB CB-CG CG-CD1 CG-CD2 CD1-CE1 CD2-CE2 CE1-CZ CE2-CZ CZ-OH",
    "TRP": "CA-CB CB-CG CG-CD1 CG-CD2 CD1-NE1 NE1-CE2 CD2-CE2 CD2-CE3 CE2-CZ2 CE3-CZ3 CZ2-CH2 CZ3-CH2"}
# Hydrogen-bond donors and acceptors among the side-chain atoms, without hydrogens.  Convention: the tautomer of histidine is unknown
# without hydrogens, so both of its ring nitrogens are donor and acceptor.  The backbone N is a donor except proline's; O and OXT
# are acceptors.
SIDE_CHAIN_DONORS = {"ARG": ("NE", "NH1", "NH2"), "ASN": ("ND2",), "GLN": ("NE2",), "LYS": ("NZ",), "TRP": ("NE1",), "SER": ("OG",),
                     "THR": ("OG1",), "TYR": ("OH",), "HIS": ("ND1", "NE2")}
SIDE_CHAIN_ACCEPTORS = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2"), "ASN": ("OD1",), "GLN": ("OE1",), "SER": ("OG",), "THR": ("OG1",),
                        "TYR": ("OH",), "HIS": ("ND1", "NE2")}
_BACKBONE_BONDS = "N-CA CA-C C-O C-OXT"


def xs_radius_table():
    """-> [21,15] float32 CPU tensor: the XS radius (C 1.9, N 1.8, O 1.7, S 2.0 A) of heavy-atom slot s of residue type t, from the
    first letter of the slot's atom name in the package's own table; 0 where the type has no such atom.  Row 20 (any type outside
    0..19) has N, CA, C, O only, as in `vdw_radius_table`."""
    from .preprocess import _tables
    names = _tables()["atom_names"]
    tab = torch.zeros(21, ENERGY_SLOTS)
    for t in range(20):
        for s in range(ENERGY_SLOTS):
            if names[t][s]:
                tab[t, s] = XS_RADIUS[names[t][s][0]]
    for s, e in enumerate(_UNK_ELEMENTS):
        tab[20, s] = XS_RADIUS[e]
    return tab


def interface_type_table():
    """-> [21,15] uint8 CPU tensor of TYPE_HYDROPHOBIC | TYPE_DONOR | TYPE_ACCEPTOR per heavy-atom slot.  Hydrophobic: a carbon none
    of whose covalent neighbours is N, O or S -- the neighbours from SIDE_CHAIN_BONDS, the backbone's bonds and the peptide bond (C is
    bonded to the next residue's N, N to the previous C); sulfur itself is not hydrophobic.  Donors and acceptors: the backbone N
    (not proline's), O, OXT, SIDE_CHAIN_DONORS and SIDE_CHAIN_ACCEPTORS.  Row 20: N (donor), CA, C, O (acceptor)."""
    from .preprocess import _tables
    t = _tables()
    tab = torch.zeros(21, ENERGY_SLOTS, dtype=torch.uint8)
    for name, side in list(SIDE_CHAIN_BONDS.items()) + [("UNK", "")]:
        r = t["res_index"][name]
        names = list(t["atom_names"][r]) if r < 20 else ["N", "CA", "C", "O"] + [""] * 11
        polar = {"N": ["C"], "C": ["N"]}                    # the peptide bond's partner elements
        for bond in (_BACKBONE_BONDS + " " + side).split():
            u, v = bond.split("-")
            if u in names and v in names:                   # (C-OXT: not in row 20)
                polar.setdefault(u, []).append(v[0])
                polar.setdefault(v, []).append(u[0])
        for s, nm in enumerate(names):
            if not nm:
                continue
            bits = 0
            if nm[0] == "C" and not any(e in "NOS" for e in polar.get(nm, [])):
                bits |= TYPE_HYDROPHOBIC
            if (nm == "N" and name != "PRO") or nm in SIDE_CHAIN_DONORS.get(name, ()):
                bits |= TYPE_DONOR
            if nm in ("O", "OXT") or nm in SIDE_CHAIN_ACCEPTORS.get(name, ()):
                bits |= TYPE_ACCEPTOR
            tab[r, s] = bits
    return tab


def _weights(weights):
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        w = ()
    if len(w) != len(ENERGY_TERMS) or not all(math.isfinite(v) for v in w):
        raise ValueError(f"weights must be five finite numbers, one per term of {ENERGY_TERMS}, got {weights!r}")
    return w


def interface_energy(pos, atom_mask, aa, group, query=None, cutoff=8.0, weights=VINA_WEIGHTS):
    """pf_interface_energy_fwd: an empirical interface energy between the atoms of residues of different `group` bytes -- the
    functional form of AutoDock Vina's scoring function (Trott & Olson, J. Comput. Chem. 2010) over heavy atoms (conventions:
    csrc/interface_energy.hip).  It is written from the publication and checked against a float64 restatement in this tree and
    against hand-computed cases; it has not been checked against the Vina program, and it is neither that program's output (no ligand
    preparation, no torsion tree, no hydrogens) nor Rosetta's dG_separated.

    pos [B,N,A,3] heavy atoms in the package's order, A >= 14, slots 0 .. min(A,15)-1 are read (pos_heavyatom passes as it is);
    atom_mask [B,N,A]; aa [B,N] residue types in the package's numbering; group [B,N] (required): only pairs of atoms whose residues
    have different group bytes are evaluated; N <= 512.  An atom takes part where its mask is set and its type has the slot
    (`xs_radius_table`).  A pair counts when r < cutoff; d = r - R_i - R_j; terms ENERGY_TERMS: gauss1 exp(-(d/0.5)^2), gauss2
    exp(-((d-3)/2)^2), repulsion d^2 for d < 0, hydrophobic (both atoms hydrophobic) 1 for d <= 0.5 falling to 0 at 1.5, hbond (a
    donor and an acceptor, `interface_type_table`) 1 for d <= -0.7 falling to 0 at 0.  query [B,N] (optional): only atoms of query
    residues are rows, every participating atom is still a partner; a participating atom that is not a row has counts -1 and zeros.
    -> dict of device tensors: terms_atom [B,N,15,5] float32 (unweighted sums per row atom), terms_residue [B,N,5], pairs_atom,
    hbond_pairs_atom, hydrophobic_pairs_atom [B,N,15] int32 (partners inside the cutoff, with hbond > 0, with hydrophobic > 0),
    energy_residue [B,N] float32 = sum_k weights[k] terms_residue[k]; terms [B,5] and energy [B] float64: each pair shows in both of
    its rows, so these are HALF the sums of terms_residue / energy_residue over all rows -- with `query` they are the plain sums
    over the query rows (for a query that is one whole group, the same number)."""
    if group is None:
        raise ValueError("interface_energy needs `group` [B,N]: the energy is that between residues of different groups")
    cutoff, w = _positive("cutoff", cutoff), _weights(weights)
    dev, (B, N, A), pos, atom_mask, (aa, group, query) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("group", group, torch.uint8), ("query", query, torch.uint8)), max_n=ENERGY_MAX_N)
    a = _capi.InterfaceEnergyArgs()
    _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, group=group, query=query)
    S, T = ENERGY_SLOTS, len(ENERGY_TERMS)
    f32 = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"terms_atom": f32(B, N, S, T), "terms_residue": f32(B, N, T), "pairs_atom": i32(B, N, S), "hbond_pairs_atom": i32(B, N, S),
           "hydrophobic_pairs_atom": i32(B, N, S), "energy_residue": f32(B, N)}
    if B and N:
        a.radius = _table("xs_radius", dev, xs_radius_table).data_ptr()
        a.types = _table("interface_types", dev, interface_type_table).data_ptr()
        _bind_out(a, out)
        work = f32(B, N, 4)                         # the residue-sized workspace: centre and extent
        a.work = work.data_ptr()
        a.B, a.N, a.n_atoms, a.cutoff = B, N, A, cutoff
        a.w_gauss1, a.w_gauss2, a.w_repulsion, a.w_hydrophobic, a.w_hbond = w
        _capi.check(_capi.load().pf_interface_energy_fwd(C.byref(a), _capi.stream_ptr()), "pf_interface_energy_fwd")
    else:
        for v in out.values():
            v.zero_()
    half = 0.5 if query is None else 1.0
    out["terms"] = out["terms_residue"].double().sum(1) * half
    out["energy"] = out["energy_residue"].double().sum(1) * half
    return out


# ---- hydrogen bonds and salt bridges ---------------------------------------------------------------------------------------------------
# Heavy-atom criteria by the published conventions: donor-acceptor distance and antecedent angles (Baker & Hubbard 1984, McDonald &
# Thornton 1994), N-O distance of a salt bridge (Barlow & Thornton 1983).  Written from the publications and checked against a float64
# restatement (tests/polar_oracle.py) and constructed cases; NOT checked against HBPLUS, PLIP or Rosetta.
POLAR_MAX_N = 512           # PF_POLAR_MAX_N
POLAR_SLOTS = 15
POLAR_MAX_PARTNERS = 4      # PF_POLAR_MAX_PARTNERS
CHARGE_CATION, CHARGE_ANION = 1, 2
CATION_NITROGENS = {"LYS": ("NZ",), "ARG": ("NE", "NH1", "NH2")}
HIS_CATION_NITROGENS = ("ND1", "NE2")       # only with his_charged
ANION_OXYGENS = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2")}


def charge_table(his_charged=False):
    """-> [21,15] uint8 CPU tensor: the charge class of heavy-atom slot s of residue type t, by atom name in the package's own table:
    CHARGE_CATION (1) for Lys NZ and Arg NE / NH1 / NH2 (with `his_charged` also His ND1 / NE2), CHARGE_ANION (2) for Asp OD1 / OD2
    and Glu OE1 / OE2, 0 elsewhere.  The termini carry no charge here.  Row 20 (any type outside 0..19): none."""
    from .preprocess import _tables
    t = _tables()
    tab = torch.zeros(21, POLAR_SLOTS, dtype=torch.uint8)
    cations = dict(CATION_NITROGENS, **({"HIS": HIS_CATION_NITROGENS} if his_charged else {}))
    for cls, by_res in ((CHARGE_CATION, cations), (CHARGE_ANION, ANION_OXYGENS)):
        for res, atoms in by_res.items():
            r = t["res_index"][res]
            for nm in atoms:
                tab[r, list(t["atom_names"][r][:POLAR_SLOTS]).index(nm)] = cls
    return tab


def antecedent_table():
    """-> [21,15,2] int8 CPU tensor: the slots of the heavy atoms bonded to slot s inside a residue of type t (`bond_table`), the two
    lowest in ascending order, -1 for none.  Every heavy atom is bonded to another of its residue, so [t,s,0] >= 0 exactly where the
    type has the slot.  No donor, acceptor or charged atom has more than two bonded heavy atoms in its residue (only carbons and
    proline's N lose a neighbour here); the peptide bond's C of the previous residue is added to N by the kernel."""
    bonds = bond_table()
    tab = torch.full((21, POLAR_SLOTS, 2), -1, dtype=torch.int8)
    for t in range(21):
        for s in range(POLAR_SLOTS):
            for k, v in enumerate(torch.nonzero(bonds[t, s]).flatten().tolist()[:2]):
                tab[t, s, k] = v
    return tab


def _cosine(name, degrees):
    try:
        v = float(degrees)
    except (TypeError, ValueError):
        v = float("nan")
    if not 0.0 <= v <= 180.0:
        raise ValueError(f"{name} must be an angle of 0 to 180 degrees, got {degrees!r}")
    return math.cos(math.radians(v))


def polar_interactions(pos, atom_mask, aa, residue_index, group=None, query=None, d_max=3.5, acc_angle_min=90.0, don_angle_min=90.0,
                       salt_max=4.0, his_charged=False):
    """pf_polar_fwd: directional hydrogen bonds and salt-bridge atom pairs between the heavy atoms of different residues, with the
    explicit list of which atom bonds which (conventions: csrc/polar.hip).  Heavy atoms only, by the published conventions: donor-
    acceptor distance and antecedent angles (Baker & Hubbard 1984, McDonald & Thornton 1994) and the N-O distance of a salt bridge
    (Barlow & Thornton 1983).  It is written from the publications and checked against a float64 restatement in this tree and against
    constructed cases; it has not been checked against HBPLUS, PLIP or Rosetta, and it is none of their outputs (no hydrogens are
    placed, histidine's tautomer is unknown, no water, no terminal charges).

    pos [B,N,A,3] heavy atoms in the package's order, A >= 14, slots 0 .. min(A,15)-1 are read; atom_mask [B,N,A]; aa [B,N] residue
    types; residue_index [B,N] (required; metrics.residue_index): consecutive residues of a chain differ by exactly 1; N <= 512.  An
    atom takes part where its mask is set and its type has the slot.  Donors and acceptors: `interface_type_table`; the antecedents
    of an atom: the participating atoms bonded to it in its residue (`antecedent_table`) and, for a backbone N, the C of the
    chain-consecutive previous row.  A hydrogen bond joins atoms of different residues, one a donor D and the other an acceptor A (both
    assignments are tried, either passing counts once), with |D - A| <= d_max, every angle X-A...D >= acc_angle_min over the
    antecedents X of A and every angle Y-D...A >= don_angle_min over the antecedents Y of D (degrees; an atom without an antecedent
    passes); the backbone N of residue i never bonds O or OXT of the chain-consecutive residue i - 1.  A salt bridge is a cation N
    and an anion O (`charge_table`; histidine's ring nitrogens only with his_charged) of different residues with |N - O| <=
    salt_max, whether or not they are hydrogen bonded.  query [B,N] (optional): only atoms of query residues are rows, every
    participating atom is still a partner; a participating atom that is not a row has counts -1 and empty lists.  group [B,N]
    (optional) adds the *_cross outputs: the partners whose residue has another group byte.
    -> dict of device tensors: hbonds_atom, salt_atom [B,N,15] int32 (partners per row atom); hbond_partner, salt_partner [B,N,15,4]
    int32 (residue * 15 + slot of the partners, ascending, the 4 lowest, -1 padded; the counts stay exact); hbonds_residue,
    salt_residue [B,N] int32; n_hbonds, n_salt_bridges [B] int64: each pair shows in both of its rows, so these are HALF the row sums
    -- with `query` the plain sums over the query rows.  With `group` every key also with `_cross` appended."""
    d_max, salt_max = _positive("d_max", d_max), _positive("salt_max", salt_max)
    cos_acc, cos_don = _cosine("acc_angle_min", acc_angle_min), _cosine("don_angle_min", don_angle_min)
    if residue_index is None:
        raise ValueError("polar_interactions needs `residue_index` [B,N] (metrics.residue_index): it tells which rows are bonded")
    dev, (B, N, A), pos, atom_mask, (aa, residue_index, group, query) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int64), ("group", group, torch.uint8),
        ("query", query, torch.uint8)), max_n=POLAR_MAX_N)
    a = _capi.PolarArgs()
    _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index, group=group, query=query)
    S, K = POLAR_SLOTS, POLAR_MAX_PARTNERS
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"hbonds_atom": i32(B, N, S), "salt_atom": i32(B, N, S), "hbond_partner": i32(B, N, S, K), "salt_partner": i32(B, N, S, K),
           "hbonds_residue": i32(B, N), "salt_residue": i32(B, N)}
    if group is not None:
        out.update(hbonds_atom_cross=i32(B, N, S), salt_atom_cross=i32(B, N, S), hbonds_residue_cross=i32(B, N),
                   salt_residue_cross=i32(B, N))
    if B and N:
        a.types = _table("interface_types", dev, interface_type_table).data_ptr()
        a.charge = _table("charge", dev, lambda: charge_table(his_charged), bool(his_charged)).data_ptr()
        a.antecedents = _table("antecedents", dev, antecedent_table).data_ptr()
        _bind_out(a, out)
        work = torch.empty(B, N, 4, device=dev)     # the residue-sized workspace: centre and extent
        a.work = work.data_ptr()
        a.B, a.N, a.n_atoms = B, N, A
        a.d_max, a.cos_acc, a.cos_don, a.salt_max = d_max, cos_acc, cos_don, salt_max
        _capi.check(_capi.load().pf_polar_fwd(C.byref(a), _capi.stream_ptr()), "pf_polar_fwd")
    else:
        for k, v in out.items():
            v.fill_(-1) if k.endswith("_partner") else v.zero_()
    div = 2 if query is None else 1
    for tag in ("", "_cross") if group is not None else ("",):
        out["n_hbonds" + tag] = out["hbonds_residue" + tag].sum(1, dtype=torch.int64) // div
        out["n_salt_bridges" + tag] = out["salt_residue" + tag].sum(1, dtype=torch.int64) // div
    return out


# A restraint force field and a monotone minimiser around it (conventions: csrc/relax.hip).  It is NOT Amber and NOT Rosetta's
# FastRelax: no hydrogens, no electrostatics, no torsion terms, no fitted parameter.  Its terms are the clash overlap and the
# peptide-bond ideals of `structural_violations` plus the input structure's own internal distances; it stands where the reference's
# evaluation relaxes a sample before scoring it (eval/energy.py, openfold/np/relax/amber_minimize.py) in role only, not in values.
RELAX_MAX_N = 512           # PF_RELAX_MAX_N
RELAX_SLOTS = 15            # PF_RELAX_SLOTS
RELAX_TERMS = ("rest", "intra", "conn", "clash")
# none of the stiffnesses is fitted to anything; k_rest is the restraint stiffness of amber_minimize.py
RELAX_DEFAULTS = dict(k_rest=10.0, k_intra=300.0, k_bond=300.0, k_angle=150.0, k_clash=200.0, clash_overlap_tolerance=1.5,
                      clash_margin=0.2, step0=0.002, gtol=0.0)


def bond_table():
    """-> [21,15,15] bool CPU tensor: the covalent bonds between the heavy-atom slots of residue type t, stated from chemistry as
    atom-name pairs (SIDE_CHAIN_BONDS and the backbone's N-CA, CA-C, C-O, C-OXT; proline's ring closes with CD-N) and resolved
    against the package's own atom-name table.  Row 20 (any type outside 0..19): N-CA, CA-C, C-O."""
    from .preprocess import _tables
    t = _tables()
    tab = torch.zeros(21, RELAX_SLOTS, RELAX_SLOTS, dtype=torch.bool)
    for name, side in list(SIDE_CHAIN_BONDS.items()) + [("UNK", "")]:
        r = t["res_index"][name]
        names = list(t["atom_names"][r][:RELAX_SLOTS]) if r < 20 else ["N", "CA", "C", "O"] + [""] * 11
        for bond in (_BACKBONE_BONDS + " " + side).split():
            u, v = bond.split("-")
            if u in names and v in names:                   # (C-OXT: not in row 20)
                tab[r, names.index(u), names.index(v)] = tab[r, names.index(v), names.index(u)] = True
    return tab


def restrained_pair_table():
    """-> [21,15,15] bool CPU tensor: the atom pairs of a residue whose distance `relax` holds at the reference's: at most two bonds
    apart in `bond_table` (bonds and bond angles), or both in the same rigid group (atom14_group of data/rigid_groups.npz; OXT counts
    with O) -- so rings and planar groups stay rigid, and psi and chi1-chi4 stay free.  Symmetric, no diagonal, existing slots only."""
    import os

    import numpy as np

    from .preprocess import _HERE, _tables
    names = _tables()["atom_names"]
    group = torch.from_numpy(np.load(os.path.join(_HERE, "data", "rigid_groups.npz"))["atom14_group"][:21]).to(torch.int64)
    group[20, 3] = group[0, 3]                              # (the file's row 20 is empty: O turns with psi there too)
    group = torch.cat([group, group[:, 3:4]], 1)            # OXT with O
    bonds = bond_table()
    two = bonds | ((bonds.to(torch.int32) @ bonds.to(torch.int32)) > 0)
    has = torch.tensor([[bool(names[t][s]) for s in range(RELAX_SLOTS)] for t in range(20)] + [[True] * 4 + [False] * 11])
    tab = (two | (group[:, :, None] == group[:, None, :])) & has[:, :, None] & has[:, None, :]
    return tab & ~torch.eye(RELAX_SLOTS, dtype=torch.bool)


def _pair_mask_table():
    """-> [21,15] int32: bit b of (t, a) = restrained_pair_table()[t, a, b], the form the kernel reads"""
    bits = (1 << torch.arange(RELAX_SLOTS, dtype=torch.int64))
    return (restrained_pair_table().to(torch.int64) * bits).sum(-1).to(torch.int32)


def _relax_params(params, steps=None):
    p = dict(RELAX_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise ValueError(f"unknown parameter {k!r}; the parameters are {tuple(p)}")
        p[k] = v
    for k in p:
        try:
            v = float(p[k])
        except (TypeError, ValueError):
            v = float("nan")
        want = "finite" if k in ("clash_overlap_tolerance", "clash_margin") else ">= 0" if k == "gtol" else "> 0"
        if not math.isfinite(v) or (want == ">= 0" and v < 0) or (want == "> 0" and not v > 0):
            raise ValueError(f"{k} must be a number {want}, got {p[k]!r}")
        p[k] = v
    if steps is not None and (not isinstance(steps, int) or isinstance(steps, bool) or steps < 0):
        raise ValueError(f"steps must be an integer >= 0, got {steps!r}")
    return p


def _relax_args(pos, ref_pos, atom_mask, aa, residue_index, movable, p):
    """the checked and bound inputs of pf_relax_energy_fwd / pf_relax_fwd -> (args, device, (B, N, A), the tensors to keep alive)"""
    if movable is None or residue_index is None:
        raise ValueError("relax needs residue_index [B,N] and movable [B,N]")
    dev, (B, N, A), pos, atom_mask, (aa, residue_index, movable) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int32), ("movable", movable, torch.uint8)), max_n=RELAX_MAX_N)
    if ref_pos is None:
        ref_pos = pos
    else:
        if not isinstance(ref_pos, torch.Tensor) or tuple(ref_pos.shape) != (B, N, A, 3):
            raise ValueError(f"ref_pos must have the shape of pos {(B, N, A, 3)}, got {tuple(getattr(ref_pos, 'shape', ()))}")
        ref_pos = _f32(ref_pos, dev)
    a = _capi.RelaxArgs()
    _bind_in(a, pos=pos, ref_pos=ref_pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index, movable=movable)
    a.B, a.N, a.n_atoms, a.pro = B, N, A, _proline()
    for k in RELAX_DEFAULTS:
        setattr(a, k, p[k])
    return a, dev, (B, N, A), [pos, ref_pos, atom_mask, aa, residue_index, movable]


def _relax_tables(a, dev):
    a.radius = _table("sasa_radius", dev, sasa_radius_table).data_ptr()
    a.pair_mask = _table("relax_pair_mask", dev, _pair_mask_table).data_ptr()


def relax_energy(pos, ref_pos, atom_mask, aa, residue_index, movable, **params):
    """pf_relax_energy_fwd: one evaluation of the restraint force field of `relax` and of its analytic gradient (conventions:
    csrc/relax.hip).  Not Amber and not Rosetta: E = E_rest + E_intra + E_conn + E_clash over heavy atoms, from the clash overlap and
    peptide-bond ideals of `structural_violations` and the internal distances of ref_pos.

    pos, ref_pos [B,N,A,3] heavy atoms in the package's order, A >= 14, slots 0 .. min(A,15)-1 are read; atom_mask [B,N,A]; aa [B,N]
    residue types; residue_index [B,N] integers (a peptide bond joins n and n + 1 where it grows by exactly 1; atoms of equal index
    never clash); movable [B,N]: the residues whose existing atoms move, every other atom is a fixed partner; N <= 512.  An atom
    exists where its mask is set and `sasa_radius_table` has the slot.  params: RELAX_DEFAULTS (k_rest, k_intra, k_bond, k_angle,
    k_clash > 0; clash_overlap_tolerance, clash_margin).
    -> dict of device tensors: terms [B,4] float64 (RELAX_TERMS: rest, intra, conn, clash), energy [B] float64, gradient [B,N,15,3]
    float32 (zero on atoms that do not move), energy_atom [B,N,15] float32, terms_atom [B,N,15,4] float32 (every pair and connection
    counted once over the atoms)."""
    p = _relax_params(params)
    a, dev, (B, N, A), keep = _relax_args(pos, ref_pos, atom_mask, aa, residue_index, movable, p)
    S, T = RELAX_SLOTS, len(RELAX_TERMS)
    f32 = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    out = {"terms": f64(B, T), "energy": f64(B), "gradient": f32(B, N, S, 3), "energy_atom": f32(B, N, S), "terms_atom": f32(B, N, S, T)}
    if B and N:
        _relax_tables(a, dev)
        _bind_out(a, out)
        work = f32(B, N, 4)                         # the residue-sized workspace: centre and extent
        a.work = work.data_ptr()
        _capi.check(_capi.load().pf_relax_energy_fwd(C.byref(a), _capi.stream_ptr()), "pf_relax_energy_fwd")
    else:
        for v in out.values():
            v.zero_()
    return out


def relax(pos, atom_mask, aa, residue_index, movable, steps=200, **params):
    """pf_relax_fwd: restrained relaxation of heavy-atom structures on the device -- `steps` iterations of a monotone steepest descent
    on the energy of `relax_energy` with ref_pos = pos (conventions: csrc/relax.hip).  It removes clashes and mends peptide bonds
    while bonds, angles and rings keep the input's geometry and every atom is tethered to where it started; it is NOT Amber
    (amber_minimize.py) and NOT Rosetta's FastRelax, and stands for them in role only.

    Arguments as `relax_energy`; steps >= 0; params: RELAX_DEFAULTS, also step0 > 0 (the first step size) and gtol >= 0.  Per sample:
    trial y = x - alpha g on the moving atoms, accepted when E(y) <= E(x) in the float64 sums (alpha *= 1.2), else rejected (alpha *=
    0.5); once max|g| <= gtol the sample is frozen.  Samples are independent of each other; nothing is read back during the loop.
    -> dict of device tensors: pos [B,N,A,3] float32 (atoms that do not move and slots >= 15 are bit-identical copies of the input);
    terms_initial, terms_final [B,4] float64; energy_trace [B,steps+1] float64 (the accepted energy after each iteration, [0]: the
    input's); accepted [B,steps] bool; step_size [B,steps] float32 (the alpha of trial i; a frozen sample repeats its last);
    grad_max [B] float32 (max|g| of the accepted state); iterations [B] int32 (iterations run before freezing); rmsd [B] float64 over
    the moving atoms against the input (0 without any)."""
    p = _relax_params(params, steps)
    a, dev, (B, N, A), keep = _relax_args(pos, None, atom_mask, aa, residue_index, movable, p)
    pos, atom_mask, aa, movable = keep[0], keep[2], keep[3], keep[5]
    S, T = RELAX_SLOTS, len(RELAX_TERMS)
    f32 = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"terms_initial": f64(B, T), "terms": f64(B, T), "energy_trace": f64(B, steps + 1),
           "accepted": torch.empty(B, steps, dtype=torch.uint8, device=dev), "step_size": f32(B, steps), "grad_max": f32(B),
           "iterations": i32(B)}
    x = f32(B, N, S, 3)
    if B and N:
        _relax_tables(a, dev)
        _bind_out(a, out)
        state = {"x": x, "g": f32(B, N, S, 3), "y": f32(B, N, S, 3), "gradient": f32(B, N, S, 3), "terms_atom": f32(B, N, S, T),
                 "work": f32(B, N, 4), "energy": f64(B), "alpha": f32(B), "frozen": i32(B)}
        _bind_out(a, state)
        a.steps = steps
        _capi.check(_capi.load().pf_relax_fwd(C.byref(a), _capi.stream_ptr()), "pf_relax_fwd")
        new = pos.clone()
        new[:, :, :S] = x[:, :, :min(A, S)]
    else:
        for v in out.values():
            v.zero_()
        new = pos.clone()
    out["terms_final"] = out.pop("terms")
    _as_bool(out, "accepted")
    tab = _table("sasa_radius", dev, sasa_radius_table)
    n = min(A, S)
    moving = (atom_mask[:, :, :n] != 0) & (tab[torch.where((aa < 0) | (aa > 20), 20, aa)][:, :, :n] > 0) & (movable != 0)[:, :, None]
    sq = ((new[:, :, :n].double() - pos[:, :, :n].double()) ** 2).sum(-1) * moving
    cnt = moving.sum((1, 2)).double()
    out["rmsd"] = torch.sqrt(sq.sum((1, 2)) / cnt.clamp(min=1.0))
    out["pos"] = new
    return out


# Rotamer side-chain packing (conventions: csrc/packing.hip).  It is NOT SCWRL4 and NOT Rosetta's packer: there is no Dunbrack library
# in this tree, the default rotamers are a staggered grid and the energy is this package's own Vina-form pair energy (`interface_energy`'s
# pair function); it stands where the reference's evaluation packs a backbone-only sample with SCWRL4 (eval/run_scwrl4.py) in role only,
# not in values.
PACK_MAX_N = 512            # PF_PACK_MAX_N
PACK_MAX_ROT = 128          # PF_PACK_MAX_ROT
PACK_SLOTS = 15             # PF_PACK_SLOTS
PACK_ROT_ATOMS = 9          # PF_PACK_ROT_ATOMS: slots 5..13
# Stated from chemistry: the chi about a bond that ends on a planar (sp2) group; every other chi is about a bond between two
# tetrahedral atoms.  Proline's ring has two puckers.
PLANAR_CHI = {"ASN": 2, "ASP": 2, "GLN": 3, "GLU": 3, "HIS": 2, "PHE": 2, "TYR": 2, "TRP": 2}
STAGGERED_DEG = (60.0, 180.0, 300.0)
PRO_ROTAMERS_DEG = ((30.0, -35.0), (-30.0, 35.0))


def rotamer_table(step_deg=30):
    """-> (chi [21,R,4] float32 radians, count [21] int32, energy [21,R] float32 zeros), CPU tensors: the default rotamers of
    `pack_sidechains`, a staggered grid and not a rotamer library.  Per residue type the product over its chi angles, chi1 slowest, each
    ascending: a chi about a bond between two tetrahedral atoms takes 60, 180, 300 degrees; the terminal planar chi (PLANAR_CHI) takes
    a step_deg grid over [0, 360), or [0, 180) where PI_PERIODIC_CHI says it is pi-periodic; PRO has the two rows PRO_ROTAMERS_DEG; ALA,
    GLY and row 20 have one empty rotamer.  R is the largest count (108 at 30 degrees, GLN); rows beyond a type's count are zero."""
    import itertools

    from .preprocess import _tables
    try:
        step = float(step_deg)
    except (TypeError, ValueError):
        step = float("nan")
    if not (math.isfinite(step) and 0.0 < step <= 180.0):
        raise ValueError(f"step_deg must be a number in (0, 180], got {step_deg!r}")
    index = _tables()["res_index"]
    n_chi = (chi_atom_table()[:, :, 0] >= 0).sum(1)
    rows = [[()] for _ in range(21)]
    for name, t in index.items():
        if t >= 20 or int(n_chi[t]) == 0:
            continue
        if name == "PRO":
            rows[t] = [tuple(r) for r in PRO_ROTAMERS_DEG]
            continue
        axes = []
        for k in range(1, int(n_chi[t]) + 1):
            if PLANAR_CHI.get(name) == k:
                period = 180.0 if PI_PERIODIC_CHI.get(name) == k else 360.0
                grid, v = [], 0.0
                while v < period - 1e-9:
                    grid.append(v)
                    v += step
                axes.append(tuple(grid))
            else:
                axes.append(STAGGERED_DEG)
        rows[t] = list(itertools.product(*axes))
    count = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    R = int(count.max())
    if R > PACK_MAX_ROT:
        raise ValueError(f"step_deg = {step_deg!r} gives {R} rotamers for one residue type; at most {PACK_MAX_ROT}")
    chi = torch.zeros(21, R, 4, dtype=torch.float64)
    for t, rs in enumerate(rows):
        for r, row in enumerate(rs):
            for k, v in enumerate(row):
                chi[t, r, k] = math.radians(v)
    return chi.to(torch.float32), count, torch.zeros(21, R, dtype=torch.float32)


def _rigid_group_table():
    """-> [21,15] int64: atom14_group of data/rigid_groups.npz, slot 14 (OXT) with O"""
    import os

    import numpy as np

    from .preprocess import _HERE
    group = torch.from_numpy(np.load(os.path.join(_HERE, "data", "rigid_groups.npz"))["atom14_group"][:21]).to(torch.int64)
    return torch.cat([group, group[:, 3:4]], 1)


def packing_pair_table():
    """-> [21,15,15] bool CPU tensor: entry (t, a, b) -- `pack_sidechains` evaluates the pair of slots a and b inside one residue of type
    t: a is a rotamer atom (slots 5..13 in a chi1..chi4 rigid group), b is more than three bonds away from it in `bond_table`, and b is
    N, CA, C, O, CB or OXT, or a rotamer atom of a smaller slot (each pair once).  Existing slots only; row 20 is empty."""
    from .preprocess import _tables
    names = _tables()["atom_names"]
    bonds = bond_table().to(torch.int32)
    eye = torch.eye(PACK_SLOTS, dtype=torch.int32)
    step = ((bonds + eye) > 0).to(torch.int32)
    within3 = (step @ step @ step) > 0
    has = torch.tensor([[bool(names[t][s]) for s in range(PACK_SLOTS)] for t in range(20)] + [[False] * PACK_SLOTS])
    rot = torch.zeros(21, PACK_SLOTS, dtype=torch.bool)
    rot[:, 5:14] = (_rigid_group_table()[:, 5:14] >= 4) & has[:, 5:14]
    a = torch.arange(PACK_SLOTS)
    fixed = (a < 5) | (a == 14)
    partner = fixed[None, None, :] | (rot[:, None, :] & (a[None, :] < a[:, None])[None])
    return rot[:, :, None] & has[:, None, :] & ~within3 & partner


def _pack_own_mask_table():
    """-> [21,15] int32: bit b of (t, a) = packing_pair_table()[t, a, b], the form the kernel reads"""
    bits = (1 << torch.arange(PACK_SLOTS, dtype=torch.int64))
    return (packing_pair_table().to(torch.int64) * bits).sum(-1).to(torch.int32)


def _check_rotamers(rotamers):
    """-> (chi [21,R,4] float32, count [21] int32, energy [21,R] float32) CPU tensors, checked (ValueError)"""
    try:
        chi, count, energy = (torch.as_tensor(v).detach().cpu() for v in rotamers)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("rotamers must be (chi [21,R,4], count [21], energy [21,R])") from None
    R = chi.shape[1] if chi.dim() == 3 else -1
    if chi.dim() != 3 or chi.shape[0] != 21 or chi.shape[2] != 4 or tuple(count.shape) != (21,) or tuple(energy.shape) != (21, R):
        raise ValueError(f"rotamers must be (chi [21,R,4], count [21], energy [21,R]), got {tuple(chi.shape)}, {tuple(count.shape)}, "
                         f"{tuple(energy.shape)}")
    if R < 1 or R > PACK_MAX_ROT:
        raise ValueError(f"a rotamer table holds 1 .. {PACK_MAX_ROT} rotamers per residue type, got R = {R}")
    count = count.to(torch.int64)
    if bool((count < 1).any()) or bool((count > R).any()):
        raise ValueError(f"rotamer counts must be in 1 .. R = {R} (count <= {PACK_MAX_ROT}), got {count.tolist()}")
    chi, energy = chi.to(torch.float32), energy.to(torch.float32)
    if not bool(torch.isfinite(chi).all()) or not bool(torch.isfinite(energy).all()):
        raise ValueError("rotamer chi and energy must be finite")
    return chi.contiguous(), count.to(torch.int32).contiguous(), energy.contiguous()


def _cysteine():
    from .preprocess import residue_type
    return residue_type("CYS")


def pack_sidechains(pos, atom_mask, aa, residue_index, movable, rotamers=None, sweeps=8, cutoff=8.0, weights=VINA_WEIGHTS, trace=False):
    """pf_pack_sidechains_fwd: rotamer side-chain packing of the movable residues on the device (conventions: csrc/packing.hip).  Every
    rotamer of a discrete table is built on the residue's own backbone (the frame of N, CA, C and the ideal rigid groups of
    `full_atom`; chi1 counts from the real N, so `torsion_angles` of the output gives `chi` back), scored with the pair function of `interface_energy` against the fixed environment, its own residue and the other
    packed residues, and one rotamer per residue is chosen by iterated conditional modes.  It is NOT SCWRL4 and NOT Rosetta's packer:
    no Dunbrack library (the default `rotamer_table` is a staggered grid), no hydrogens, no fitted parameter, a deterministic local
    search and not the global minimum; it stands for them in role only.

    Arguments as `relax`: pos [B,N,A,3], A >= 14; atom_mask [B,N,A]; aa [B,N]; residue_index [B,N]; movable [B,N]; N <= 512.  A
    movable residue of a type in 0..19 whose N, CA and C are in atom_mask is packed; every other residue is fixed environment and
    comes back bit for bit.  rotamers: (chi [21,R,4] radians, count [21], energy [21,R]) with R, count <= 128, e.g. a real library
    with energy = -log p; None: `rotamer_table()`.  sweeps >= 0; cutoff and weights as `interface_energy`.
    -> dict of device tensors: pos [B,N,15,3] float32 and atom_mask [B,N,15] bool (packed residues: N, CA, C, O and slot 14 as given,
    CB rebuilt, slots 4..13 of the mask the type's); packed [B,N] bool; rotamer [B,N] int32 (-1 where not packed); chi [B,N,4] float32
    (the chosen row); n_rotamers [B,N] int32; energy_self_best [B,N] float32 (the smallest E_self: the start); energy_residue [B,N]
    float32 (E_self plus half of each of the residue's pair terms at the end); energy_trace [B,sweeps+1] float64 (the total after each
    sweep, [0]: the start; sweeps not run repeat the last); sweeps_run [B] int32; changed [B,sweeps] int32 (rotamers changed in each
    sweep); with trace=True also choice_trace [B,sweeps,N] int32 (the rotamer taken at each visit, -1 where none)."""
    if movable is None or residue_index is None:
        raise ValueError("pack_sidechains needs residue_index [B,N] and movable [B,N]")
    if not isinstance(sweeps, int) or isinstance(sweeps, bool) or sweeps < 0:
        raise ValueError(f"sweeps must be an integer >= 0, got {sweeps!r}")
    cutoff, w = _positive("cutoff", cutoff), _weights(weights)
    rot = None if rotamers is None else _check_rotamers(rotamers)
    dev, (B, N, A), pos, atom_mask, (aa, residue_index, movable) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int32), ("movable", movable, torch.uint8)), max_n=PACK_MAX_N)
    S = PACK_SLOTS
    f32 = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731
    i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"pos": f32(B, N, S, 3), "atom_mask": torch.zeros(B, N, S, dtype=torch.uint8, device=dev),
           "packed": torch.zeros(B, N, dtype=torch.uint8, device=dev), "rotamer": i32(B, N, fill=-1), "chi": f32(B, N, 4),
           "n_rotamers": i32(B, N), "energy_self_best": f32(B, N), "energy_residue": f32(B, N),
           "energy_trace": torch.zeros(B, sweeps + 1, dtype=torch.float64, device=dev), "sweeps_run": i32(B), "changed": i32(B, sweeps)}
    if trace:
        out["choice_trace"] = i32(B, sweeps, N, fill=-1)
    if B and N:
        from . import full_atom
        if rot is None:
            tabs = [_table("rotamer_" + k, dev, lambda k=k: dict(zip(("chi", "count", "energy"), rotamer_table()))[k])
                    for k in ("chi", "count", "energy")]
        else:
            tabs = [t.to(dev) for t in rot]
        R = tabs[0].shape[1]
        rigid, frames = full_atom._tables(dev)
        if frames != [3, 4, 5, 6, 7]:
            raise _capi.PepflowHipError(f"rigid_groups.npz: the frames are {frames}, the packing kernel is written for [3, 4, 5, 6, 7]")
        lib = _capi.load()
        nbytes = lib.pf_pack_work_bytes(B, N, R)
        if nbytes < 0:
            raise ValueError(f"pack_sidechains: the workspace for B = {B}, N = {N}, {R} rotamers exceeds 2 GiB; pack the batch in parts")
        a = _capi.PackArgs()
        _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index, movable=movable)
        a.radius = _table("xs_radius", dev, xs_radius_table).data_ptr()
        a.types = _table("interface_types", dev, interface_type_table).data_ptr()
        a.own_mask = _table("pack_own_mask", dev, _pack_own_mask_table).data_ptr()
        a.tab_rot, a.tab_trans, a.tab_group, a.tab_pos, a.tab_mask = (rigid[k].data_ptr() for k in ("rot", "trans", "group", "pos", "mask"))
        a.rot_chi, a.rot_count, a.rot_energy = (t.data_ptr() for t in tabs)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        a.work = work.data_ptr()
        _bind_out(a, {("mask_out" if k == "atom_mask" else "pos_out" if k == "pos" else k): v for k, v in out.items()})
        a.B, a.N, a.n_atoms, a.max_rot, a.sweeps, a.pro, a.cys = B, N, A, R, sweeps, _proline(), _cysteine()
        a.cutoff = cutoff
        a.w_gauss1, a.w_gauss2, a.w_repulsion, a.w_hydrophobic, a.w_hbond = w
        _capi.check(lib.pf_pack_sidechains_fwd(C.byref(a), _capi.stream_ptr()), "pf_pack_sidechains_fwd")
    _as_bool(out, "atom_mask", "packed")
    return out


# Point-mutation scanning (conventions: csrc/mutscan.hip).  It is NOT FoldX (which the reference's eval/foldx.py calls; its main uses
# are AlaScan and PositionScan) and NOT Rosetta: the energy is `pack_sidechains`' E_self on an unmoved, unrepacked environment.
SCAN_TYPES = 20             # PF_MUTATION_SCAN_TYPES: the candidate residue types 0..19


def _scan_candidates(candidates, B, N):
    """None (every type), a [20] mask or a [B,N,20] mask -> None or a [B,N,20] bool tensor (ValueError)"""
    if candidates is None:
        return None
    c = torch.as_tensor(candidates)
    if tuple(c.shape) == (SCAN_TYPES,):
        c = c.reshape(1, 1, SCAN_TYPES).expand(B, N, SCAN_TYPES)
    if tuple(c.shape) != (B, N, SCAN_TYPES):
        raise ValueError(f"candidates must be None, [{SCAN_TYPES}] or [B,N,{SCAN_TYPES}] = {(B, N, SCAN_TYPES)}, got {tuple(c.shape)}")
    return c != 0


def mutation_scan(pos, atom_mask, aa, residue_index, positions, candidates=None, group=None, rotamers=None, cutoff=8.0,
                  weights=VINA_WEIGHTS):
    """pf_mutation_scan_fwd: single-point mutants of the residues `positions` on the device (conventions: csrc/mutscan.hip).  At each
    scanned residue q and for each candidate type t, every rotamer of t is built on q's own backbone as `pack_sidechains` builds it
    and scored with its E_self: against every other residue exactly as given (side chains included; neighbours are not repacked and
    other scanned positions stay as they are), against the own residue with type t's atoms, and the table's energy; the smallest is
    kept.  ddE[q,t] = energy[q,t] - energy[q,aa[q]]: the wild type is repacked on the same rotamer grid, so ddE is exactly 0 at t =
    aa[q].  energy[q,t] has the bits of `pack_sidechains(aa with aa[q] := t, movable = onehot(q), sweeps=0)["energy_self_best"][q]`.

    What the numbers are, and are not: ALA and GLY have no rotamer atom, so both score the table's energy (0 by default), and
    ddE[q,ALA] is minus the contribution of q's side chain beyond CB, which is what an alanine scan reports; differences in the
    backbone (PRO's N, GLY's missing CB) do not show; there is no solvation, no electrostatics, no entropy and no backbone movement.
    It is NOT FoldX and NOT Rosetta, and it stands for their AlaScan / PositionScan in role only; the defaults are untuned.

    Arguments as `pack_sidechains` with positions [B,N] in place of movable: a residue is scanned where positions is set, its type is
    in 0..19 and its N, CA and C are in atom_mask.  candidates: None (all 20 types), a [20] mask or a [B,N,20] mask; the wild type is
    evaluated at every scanned residue whatever the mask says.  group [B,N] (optional): energy_interface counts only partners whose
    group differs from the residue's.  rotamers, cutoff, weights as `pack_sidechains`.
    -> dict of device tensors: scanned [B,N] bool; energy [B,N,20] float32 (+inf where not evaluated); rotamer [B,N,20] int32 (-1);
    n_rotamers [B,N,20] int32 (0); chi [B,N,20,4] float32 (the chosen row); energy_interface [B,N,20] float32 (the chosen rotamer's
    pair terms against residues of another group; 0 without group, +inf where not evaluated); ddE and ddE_interface [B,N,20] float32
    (NaN where either side is not evaluated)."""
    if positions is None or residue_index is None:
        raise ValueError("mutation_scan needs residue_index [B,N] and positions [B,N]")
    cutoff, w = _positive("cutoff", cutoff), _weights(weights)
    rot = None if rotamers is None else _check_rotamers(rotamers)
    dev, (B, N, A), pos, atom_mask, (aa, residue_index, positions, group) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int32), ("positions", positions, torch.uint8),
        ("group", group, torch.uint8)), max_n=PACK_MAX_N)
    cand = _scan_candidates(candidates, B, N)
    cand = None if cand is None else _bytes(cand, dev)
    T = SCAN_TYPES
    out = {"scanned": torch.zeros(B, N, dtype=torch.uint8, device=dev), "energy": torch.full((B, N, T), float("inf"), device=dev),
           "rotamer": torch.full((B, N, T), -1, dtype=torch.int32, device=dev),
           "n_rotamers": torch.zeros(B, N, T, dtype=torch.int32, device=dev), "chi": torch.zeros(B, N, T, 4, device=dev),
           "energy_interface": torch.full((B, N, T), float("inf"), device=dev)}
    if B and N:
        from . import full_atom
        if rot is None:
            tabs = [_table("rotamer_" + k, dev, lambda k=k: dict(zip(("chi", "count", "energy"), rotamer_table()))[k])
                    for k in ("chi", "count", "energy")]
        else:
            tabs = [t.to(dev) for t in rot]
        R = tabs[0].shape[1]
        rigid, frames = full_atom._tables(dev)
        if frames != [3, 4, 5, 6, 7]:
            raise _capi.PepflowHipError(f"rigid_groups.npz: the frames are {frames}, the scan kernel is written for [3, 4, 5, 6, 7]")
        lib = _capi.load()
        nbytes = lib.pf_mutation_scan_work_bytes(B, N)
        if nbytes < 0:
            raise ValueError(f"mutation_scan: the workspace for B = {B}, N = {N} exceeds 2 GiB; scan the batch in parts")
        a = _capi.MutationScanArgs()
        _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index, positions=positions, candidates=cand, group=group)
        a.radius = _table("xs_radius", dev, xs_radius_table).data_ptr()
        a.types = _table("interface_types", dev, interface_type_table).data_ptr()
        a.own_mask = _table("pack_own_mask", dev, _pack_own_mask_table).data_ptr()
        a.tab_rot, a.tab_trans, a.tab_group, a.tab_pos, a.tab_mask = (rigid[k].data_ptr() for k in ("rot", "trans", "group", "pos", "mask"))
        a.rot_chi, a.rot_count, a.rot_energy = (t.data_ptr() for t in tabs)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        a.work = work.data_ptr()
        _bind_out(a, out)
        a.B, a.N, a.n_atoms, a.max_rot, a.pro, a.cys = B, N, A, R, _proline(), _cysteine()
        a.cutoff = cutoff
        a.w_gauss1, a.w_gauss2, a.w_repulsion, a.w_hydrophobic, a.w_hbond = w
        _capi.check(lib.pf_mutation_scan_fwd(C.byref(a), _capi.stream_ptr()), "pf_mutation_scan_fwd")
    _as_bool(out, "scanned")
    # ddE on the device: against the wild type's own entry; NaN where either side was not evaluated
    done = out["rotamer"] >= 0
    wt = aa.clamp(0, T - 1)[:, :, None]
    ok = done & torch.gather(done, 2, wt)
    nan = torch.full((), float("nan"), device=dev)
    for k, src in (("ddE", "energy"), ("ddE_interface", "energy_interface")):
        out[k] = torch.where(ok, out[src] - torch.gather(out[src], 2, wt), nan)
    return out


# Fixed-backbone sequence design (conventions: csrc/seqdesign.hip).  It is NOT ProteinMPNN (which the reference's eval/run_mpnn.py runs
# over backbone-only samples) and NOT Rosetta fixbb: an iterated-conditional-modes search over type and rotamer with `pack_sidechains`'
# own energy, no learned prior; it stands for them in role only.
SEQ_DESIGN_MAX_RES = 64     # PF_SEQ_DESIGN_MAX_RES: designed residues per sample
SEQ_DESIGN_TYPES = 20       # PF_SEQ_DESIGN_TYPES: the candidate residue types 0..19


def _ref_energy(ref_energy):
    """None or 20 finite numbers -> None or a [20] float32 CPU tensor (ValueError)"""
    if ref_energy is None:
        return None
    try:
        r = torch.as_tensor(ref_energy).detach().cpu().to(torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"ref_energy must be None or {SEQ_DESIGN_TYPES} finite numbers, got {ref_energy!r}") from None
    if tuple(r.shape) != (SEQ_DESIGN_TYPES,):
        raise ValueError(f"ref_energy must be None or {SEQ_DESIGN_TYPES} finite numbers, got shape {tuple(r.shape)}")
    if not bool(torch.isfinite(r).all()):
        raise ValueError(f"ref_energy must be finite, got {r.tolist()}")
    return r.contiguous()


def design_sequence(pos, atom_mask, aa, residue_index, designed, candidates=None, ref_energy=None, rotamers=None, sweeps=8, cutoff=8.0,
                    weights=VINA_WEIGHTS, trace=False):
    """pf_sequence_design_fwd: fixed-backbone sequence design of the residues `designed` on the device (conventions: csrc/
    seqdesign.hip).  The residue type AND the rotamer of every designed residue are chosen together by iterated conditional modes:
    every rotamer of every candidate type is built on the residue's own backbone as `pack_sidechains` builds it; its energy is
    `mutation_scan`'s E_self against the residues that are not designed (plus ref_energy[type]), plus the pair terms with the other
    designed residues in their current types and rotamers -- CB, radii and type bits follow the current type -- and a sweep gives
    every designed residue, in ascending position, the (type, rotamer) of smallest conditional energy.  Every accepted move lowers
    the total energy; the search stops after a sweep that changed nothing, or after `sweeps`.

    What it is, and is not: it stands where the reference's evaluation runs ProteinMPNN over backbone-only samples (eval/
    run_mpnn.py), in role only.  It is NOT ProteinMPNN and NOT Rosetta fixbb: the energy is this package's Vina-form pair energy plus
    the rotamer table's energy plus `ref_energy`; there is no solvation, no electrostatics, no entropy and no learned prior, and the
    backbone does not move.  Without reference energies the energy favours large side chains (more atoms, more attractive pairs);
    ref_energy is the caller's and none is shipped.  A deterministic local search, not the global minimum; the defaults are untuned.

    Arguments as `pack_sidechains` with designed [B,N] in place of movable: a residue is designed where `designed` is set, its type
    is in 0..19 and its N, CA and C are in atom_mask; every other residue is fixed environment and comes back bit for bit.
    candidates: None (all 20 types), a [20] mask or a [B,N,20] mask; a residue whose set is empty keeps its type and is repacked.
    ref_energy: None or 20 finite numbers added to the energy of every rotamer of the type.  At most SEQ_DESIGN_MAX_RES = 64
    residues are designed in a sample: a sample with more gets status 1 and comes back as if nothing were designed (decided on the
    device).  rotamers, sweeps, cutoff, weights as `pack_sidechains`.
    -> dict of device tensors: aa [B,N] int64 (the designed types; others as given); pos [B,N,15,3] float32 and atom_mask [B,N,15]
    bool as `pack_sidechains`; designed [B,N] bool; status [B] int32; rotamer [B,N] int32 (-1); chi [B,N,4] float32; n_candidates
    [B,N] int32; energy_self_best [B,N] float32 (E_self of the start); energy_residue [B,N] float32 (E_self plus half the pair terms
    at the end); energy_trace [B,sweeps+1] float64 ([0]: the start; sweeps not run repeat the last); sweeps_run [B] int32; changed,
    changed_types [B,sweeps] int32 (residues whose (type, rotamer), whose type changed in each sweep); profile [B,N,20] float32 (the
    smallest conditional energy of each candidate type against the final state of the others; +inf for a non-candidate) and
    profile_rotamer [B,N,20] int32 (-1); with trace=True also choice_trace [B,sweeps,N,2] int32 (type and rotamer taken at each
    visit, -1 where none)."""
    if designed is None or residue_index is None:
        raise ValueError("design_sequence needs residue_index [B,N] and designed [B,N]")
    if not isinstance(sweeps, int) or isinstance(sweeps, bool) or sweeps < 0:
        raise ValueError(f"sweeps must be an integer >= 0, got {sweeps!r}")
    cutoff, w = _positive("cutoff", cutoff), _weights(weights)
    rot = None if rotamers is None else _check_rotamers(rotamers)
    ref = _ref_energy(ref_energy)
    dev, (B, N, A), pos, atom_mask, (aa, residue_index, designed) = _structure(pos, atom_mask, (
        ("aa", aa, torch.int64), ("residue_index", residue_index, torch.int32), ("designed", designed, torch.uint8)), max_n=PACK_MAX_N)
    cand = _scan_candidates(candidates, B, N)
    cand = None if cand is None else _bytes(cand, dev)
    S, T = PACK_SLOTS, SEQ_DESIGN_TYPES
    f32 = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731
    i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"aa": torch.zeros(B, N, dtype=torch.int64, device=dev), "pos": f32(B, N, S, 3),
           "atom_mask": torch.zeros(B, N, S, dtype=torch.uint8, device=dev), "designed": torch.zeros(B, N, dtype=torch.uint8, device=dev),
           "status": i32(B), "rotamer": i32(B, N, fill=-1), "chi": f32(B, N, 4), "n_candidates": i32(B, N),
           "energy_self_best": f32(B, N), "energy_residue": f32(B, N),
           "energy_trace": torch.zeros(B, sweeps + 1, dtype=torch.float64, device=dev), "sweeps_run": i32(B), "changed": i32(B, sweeps),
           "changed_types": i32(B, sweeps), "profile": torch.full((B, N, T), float("inf"), device=dev),
           "profile_rotamer": i32(B, N, T, fill=-1)}
    if trace:
        out["choice_trace"] = i32(B, sweeps, N, 2, fill=-1)
    if B and N:
        from . import full_atom
        if rot is None:
            tabs = [_table("rotamer_" + k, dev, lambda k=k: dict(zip(("chi", "count", "energy"), rotamer_table()))[k])
                    for k in ("chi", "count", "energy")]
        else:
            tabs = [t.to(dev) for t in rot]
        R = tabs[0].shape[1]
        rigid, frames = full_atom._tables(dev)
        if frames != [3, 4, 5, 6, 7]:
            raise _capi.PepflowHipError(f"rigid_groups.npz: the frames are {frames}, the design kernel is written for [3, 4, 5, 6, 7]")
        lib = _capi.load()
        nbytes = lib.pf_sequence_design_work_bytes(B, N, R, SEQ_DESIGN_MAX_RES)
        if nbytes < 0:
            raise ValueError(f"design_sequence: the workspace for B = {B}, N = {N}, {R} rotamers exceeds 2 GiB; design the batch in parts")
        ref = None if ref is None else ref.to(dev)
        a = _capi.SeqDesignArgs()
        _bind_in(a, pos=pos, atom_mask=atom_mask, aa=aa, residue_index=residue_index, designed=designed, candidates=cand, ref_energy=ref)
        a.radius = _table("xs_radius", dev, xs_radius_table).data_ptr()
        a.types = _table("interface_types", dev, interface_type_table).data_ptr()
        a.own_mask = _table("pack_own_mask", dev, _pack_own_mask_table).data_ptr()
        a.tab_rot, a.tab_trans, a.tab_group, a.tab_pos, a.tab_mask = (rigid[k].data_ptr() for k in ("rot", "trans", "group", "pos", "mask"))
        a.rot_chi, a.rot_count, a.rot_energy = (t.data_ptr() for t in tabs)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        a.work = work.data_ptr()
        names = {"aa": "aa_out", "pos": "pos_out", "atom_mask": "mask_out", "designed": "designed_out"}
        _bind_out(a, {names.get(k, k): v for k, v in out.items()})
        a.B, a.N, a.n_atoms, a.max_rot, a.max_res, a.sweeps, a.pro, a.cys = B, N, A, R, SEQ_DESIGN_MAX_RES, sweeps, _proline(), _cysteine()
        a.cutoff = cutoff
        a.w_gauss1, a.w_gauss2, a.w_repulsion, a.w_hydrophobic, a.w_hbond = w
        _capi.check(lib.pf_sequence_design_fwd(C.byref(a), _capi.stream_ptr()), "pf_sequence_design_fwd")
    _as_bool(out, "atom_mask", "designed")
    return out


# Guiding potentials of the sampler on their own (conventions and formulas: csrc/guidance.hip, include/pepflow_hip.h).  They stand
# where RFdiffusion's guiding potentials stand, in role only: written from their formulas, checked against no other program.
CA_POTENTIAL_MAX_L = _capi.GUIDE_MAX_L


def ca_potential(x, peptide, movable, context, hotspots=None, restraints=None, t=1.0, **params):
    """pf_guidance_fwd in its stand-alone mode: the five C-alpha potentials `FlowModel.sample(guide=...)` steers with, and their
    gradient, evaluated once on given positions.

    x [B,L,3] C-alpha positions in Angstrom (device tensor); peptide, movable, context: bool [B,L] -- the peptide rows, the ones among
    them that may move (a subset of peptide) and the context rows (disjoint from peptide); rows in neither take no part.  hotspots:
    bool [L] or [B,L], context rows; restraints: one list for all samples, or one list per sample, of (i, j, lo, hi, weight), at most
    64.  t: the flow time the shift's schedule is evaluated at, a number or [B].  params: the entries of `sample()`'s guide dict
    (sampler.GUIDE_DEFAULTS: weights, r_receptor, r_self, min_sep, bond_tol, r_hotspot, beta, scale, t_on, power, max_shift).
    -> dict of device tensors: energy [B,5] (sampler.GUIDE_TERMS: receptor_clash, self_clash, ca_bond, hotspot, restraint), grad [B,L,3]
    (dE/dx on movable rows, zero elsewhere), guided [B,L,3] (x - the clipped shift on movable rows, the bits of x elsewhere),
    shift_max [B]."""
    from . import sampler as S
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"x must be a tensor [B,L,3], got {tuple(getattr(x, 'shape', ()))}")
    B, L = x.shape[:2]
    if L > CA_POTENTIAL_MAX_L:
        raise ValueError(f"L = {L}: at most {CA_POTENTIAL_MAX_L} residues")
    masks = {}
    for name, m in (("peptide", peptide), ("movable", movable), ("context", context)):
        if not isinstance(m, torch.Tensor) or m.dtype != torch.bool or tuple(m.shape) != (B, L):
            raise ValueError(f"{name} must be a bool tensor [{B},{L}], got {getattr(m, 'dtype', type(m).__name__)} {tuple(getattr(m, 'shape', ()))}")
        masks[name] = m.detach().cpu()
    if bool((masks["movable"] & ~masks["peptide"]).any()):
        raise ValueError("movable must be a subset of peptide")
    if bool((masks["context"] & masks["peptide"]).any()):
        raise ValueError("context and peptide must be disjoint")
    guide = S.make_guide({**params, "hotspots": hotspots, "restraints": restraints}, B, L, masks["peptide"], masks["peptide"] | masks["context"])
    dev = x.device
    x = _f32(x, dev)
    tt = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    if tt.numel() not in (1, B):
        raise ValueError(f"t must be a number or [{B}] values, got {tt.numel()}")
    tt = tt.expand(B).contiguous().to(dev)
    f32 = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
    out = {"energy": f32(B, _capi.GUIDE_NTERMS), "grad": f32(B, L, 3), "guided": f32(B, L, 3), "shift_max": f32(B)}
    if not (B and L):
        for v in out.values():
            v.zero_()
        return out
    gen, res = _f32(masks["peptide"], dev), _f32(masks["peptide"] | masks["context"], dev)
    flags = _bytes(masks["movable"], dev)
    keep = {k: (None if v is None else v.to(dev).contiguous()) for k, v in guide.items()}
    err = torch.zeros(B, dtype=torch.int32, device=dev)
    a = _capi.GuidanceArgs()
    _bind_in(a, pred_trans=x, trans1=x, gen_mask=gen, res_mask=res, res_flags=flags, hotspots=keep["hotspots"],
             pair_idx=keep["pair_idx"], pair_par=keep["pair_par"], params=keep["params"], t=tt)
    a.guided_trans, a.energy, a.shift_max, a.grad, a.error = (out["guided"].data_ptr(), out["energy"].data_ptr(), out["shift_max"].data_ptr(),
                                                            out["grad"].data_ptr(), err.data_ptr())
    a.B, a.L, a.num_steps, a.sample_bb = B, L, 0, 1
    _capi.check(_capi.load().pf_guidance_fwd(C.byref(a), _capi.stream_ptr()), "pf_guidance_fwd")
    if bool((err != 0).any()):
        raise _capi.PepflowHipError("pf_guidance_fwd refused a restraint index outside the sample")
    return out


def resample_particles(logw, groups=None, u=None, ess_frac=1.0, seed=0, state=None):
    """pf_sampler_steer in its stand-alone mode: one adaptive systematic resampling decision per particle group, as
    `FlowModel.sample(steer=...)` takes it after a step.

    logw [B] log-weights (device tensor; -inf and NaN count as weight 0); groups: None (one group) or an integer tensor [B] of arbitrary
    labels, at most 1024 members each; u: None (Philox4x32-10 with `seed`, keyed by the group's first member) or [G] uniforms in [0, 1),
    one per group in the order of the groups' first members; ess_frac in [0, 1]: a group is resampled iff its effective sample size is
    at most ess_frac * n (1: always, 0: never).  state: None, or the seven per-particle tensors (rot_t [B,L,9], trans_t [B,L,3], ang_t
    [B,L,5], seq_t int64 [B,L], simplex_t [B,L,20], trans0 [B,L,3], simplex0 [B,L,20]; contiguous device tensors) to gather IN PLACE.
    -> dict of device tensors: ancestors int64 [B] (the sample every slot continues from; sources are surviving slots), ess float64 [G],
    code int32 [G] (1 not resampled, 2 resampled, -1 no finite weight), logw float64 [B] (0 in a resampled group), groups int64 [B]."""
    import numpy as np
    from . import sampler as S
    if not isinstance(logw, torch.Tensor) or logw.dim() != 1:
        raise ValueError(f"logw must be a tensor [B], got {tuple(getattr(logw, 'shape', ()))}")
    B, dev = logw.shape[0], logw.device
    _capi.dptr(logw, logw.dtype, "logw")                       # a CPU tensor raises: no fallback
    if isinstance(ess_frac, bool) or not 0.0 <= float(ess_frac) <= 1.0:
        raise ValueError(f"ess_frac = {ess_frac!r}: expected a number in [0, 1]")
    if groups is not None and (not isinstance(groups, torch.Tensor) or groups.dtype.is_floating_point or groups.dtype == torch.bool or tuple(groups.shape) != (B,)):
        raise ValueError(f"groups: expected None or an integer tensor [{B}]")
    if B == 0:
        raise ValueError("logw is empty")
    ptr, members, group_of, G = S.pack_groups(np.zeros(B, dtype=np.int64) if groups is None else groups.detach().cpu().numpy())
    sizes = np.diff(ptr[:G + 1])
    if sizes.max() > _capi.STEER_MAX_GROUP:
        raise ValueError(f"group {int(sizes.argmax())} has {int(sizes.max())} members; at most {_capi.STEER_MAX_GROUP}")
    keep = {"params": torch.tensor([0.0, 1.0, float(ess_frac), 0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev),
            "group_ptr": torch.from_numpy(ptr).to(dev), "members": torch.from_numpy(members).to(dev),
            "n_groups": torch.tensor([G], dtype=torch.int32, device=dev), "energy": torch.zeros(B, 5, device=dev),
            "logw": logw.detach().to(torch.float64).clone().contiguous()}
    out = {"ancestors": torch.arange(B, dtype=torch.int32, device=dev), "ess": torch.zeros(G, dtype=torch.float64, device=dev),
           "code": torch.zeros(G, dtype=torch.int32, device=dev)}
    a = _capi.SamplerSteerArgs()
    _bind_in(a, **keep, **out)
    if u is not None:
        uu = torch.as_tensor(u, dtype=torch.float64).reshape(-1)
        if uu.numel() != G or not bool(((uu >= 0) & (uu < 1)).all()):
            raise ValueError(f"u: expected {G} values in [0, 1), one per group")
        keep["u"] = uu.to(dev).contiguous()
        a.u = keep["u"].data_ptr()
    L = 1
    if state is not None:
        names = ("rot_t", "trans_t", "ang_t", "seq_t", "simplex_t", "trans0", "simplex0")
        if len(state) != 7:
            raise ValueError(f"state: expected the seven tensors {names}")
        L = state[0].shape[1]
        for name, v, wd in zip(names, state, (9, 3, 5, 1, 20, 3, 20)):
            want = torch.int64 if name == "seq_t" else torch.float32
            if not isinstance(v, torch.Tensor) or v.dtype != want or v.device != dev or not v.is_contiguous() or v.numel() != B * L * wd or v.shape[0] != B:
                raise ValueError(f"state {name}: expected a contiguous {want} tensor [{B}, {L}, {wd}] on {dev}")
            setattr(a, name, _capi.dptr(v, want, name))
    a.seed, a.first_sample, a.B, a.L, a.num_steps, a.max_group = int(seed) & (2 ** 64 - 1), 0, B, L, 1, int(sizes.max())
    _capi.check(_capi.load().pf_sampler_steer(C.byref(a), _capi.stream_ptr()), "pf_sampler_steer")
    return {"ancestors": out["ancestors"].to(torch.int64), "ess": out["ess"], "code": out["code"], "logw": keep["logw"],
            "groups": torch.from_numpy(group_of).to(dev, torch.int64)}
