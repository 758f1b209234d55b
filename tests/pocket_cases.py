"""PDB-shaped inputs of encode(): named, seeded batches in the schema `model.encode` takes (host code only, numpy / torch).

`pepflowww_amd.synth.make_pocket_batch` always builds one topology: receptor first, peptide last, `res_nb` 1..n without a gap, two chain
ids, a suffix `generate_mask`, canonical atom masks, no UNK in the context, trailing padding.  The reference feeds the featurisers a
`pocket.pdb` (models_con/pep_dataloader.py:41-71): fragments of several chains with PDB numbering, missing atoms, UNK residues.  The
cases here take the GEOMETRY of `synth.make_pocket` and edit the TOPOLOGY so that every data-dependent branch of
pf_node_features_fwd / pf_edge_features_fwd / pf_edge_index is driven:

  * receptor fragments: three to five over two or three chains (`chain_nb` 1..3, peptide 0), `res_nb` from PDB-like starts (one above
    1000, one negative, one crossing 0), gaps from 1 (d == 2) over 32 / 33 to far above the clamp, one fragment numbered downwards
    (d == -1), one repeated number (insertion code, d == 0), equal numbers on different chains;
  * missing atoms (mask False, position 0 as the parser leaves them): random side-chain atoms, one context residue without N, one
    without C, one without CA (so `mres` is False INSIDE a sample while N and C are there), one context residue of type UNK (20);
  * the peptide in the middle with context at both ends, a peptide of one residue, a full-length sample with L % 16 != 0 whose
    first and last residues are context (NodeEmbedder's rolled dihedral mask wraps there), a padded and a fully padded sample;
  * `collinear`: backbone atoms placed so that p0, p1, p2 of a dihedral are EXACTLY collinear (u1 == 0) while the rounding of
    (v1 x v2) . v0 leaves a non-zero sign: the reference's clamp keeps the NaN cosine and nan_to_num makes the angle 0.

Every case is checked here for conditioning: wherever N, CA or C of a residue is present, |C - CA| and the component of N - CA
orthogonal to it exceed 0.5 A, so the 1e-6 of construct_3d_basis (geometry.py:89-111) never amplifies rounding.  All-zero rows
(padding) are exact and stay.
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(_HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(_HERE))
from pepflowww_amd import synth  # noqa: E402  (host-side data generation only)

PAD_AA, UNK_AA = 21, 20
BB_N, BB_CA, BB_C = 0, 1, 2
COLLINEAR_V0 = (1.25, 0.75, -2.5)          # exactly representable, as are its multiples and the grid points below


def up(start, n):
    return list(range(start, start + n))


def down(start, n):
    return list(range(start, start - n, -1))


# case -> (L, seed, [sample]); sample = dict(pep=(first, count), frags=[(chain, [res_nb ...]) ...] in residue order around the peptide,
# noN / noC / noCA / unk = index of the context residue edited that way).  A sample's length is what its fragments and peptide add up to.
_SPECS = {
    "frag19": (19, 3101, [
        dict(pep=(7, 5), frags=[(1, up(1043, 4)), (1, up(1048, 3)), (2, down(-3, 4)), (2, [57, 57, 58])], noN=2, noC=13, noCA=16, unk=5),
        dict(pep=(6, 1), frags=[(1, up(-2, 6)), (3, up(2, 4)), (1, up(40, 3))], noN=9, noC=1, noCA=3, unk=11),
    ]),
    "frag33": (33, 3201, [
        dict(pep=(12, 8), frags=[(1, up(95, 6)), (1, up(122, 6)), (2, down(1210, 5)), (3, [7, 8, 8, 9]), (2, up(-12, 4))],
             noN=3, noC=22, noCA=8, unk=27),
        dict(pep=(1, 4), frags=[(1, [300]), (1, up(302, 8)), (2, up(300, 7)), (3, down(50, 7))], noN=7, noC=15, noCA=20, unk=24),
        dict(pep=(10, 6), frags=[(2, up(1, 5)), (2, up(7, 2)), (2, up(14, 3)), (1, up(70, 4))], noN=17, noC=4, noCA=2, unk=8),
    ]),
    "wrap40": (40, 3301, [
        dict(pep=(10, 6), frags=[(1, up(210, 10)), (1, up(221, 8)), (2, up(1001, 8)), (3, down(-1, 8))], noN=20, noC=5, noCA=28, unk=35),
        dict(pep=(8, 4), frags=[(1, up(5, 8)), (2, up(5, 8))], noN=2, noC=14, noCA=17, unk=5),
    ]),
    # a caller batch of 40 whose second sample FILLS its 32-residue length bucket with context at both ends: residue 0's wrapped
    # neighbour is the caller's residue 39 (padding), not row 31 of the bucket's launch
    "cut40": (40, 3701, [
        dict(pep=(10, 6), frags=[(1, up(210, 10)), (1, up(221, 8)), (2, up(1001, 8)), (3, down(-1, 8))], noN=20, noC=5, noCA=28, unk=35),
        dict(pep=(12, 6), frags=[(1, up(5, 12)), (2, up(5, 8)), (3, down(-1, 6))], noN=3, noC=20, noCA=24, unk=8),
    ]),
    "pad48": (48, 3401, [
        dict(pep=(20, 10), frags=[(1, up(400, 10)), (1, up(433, 10)), (2, down(90, 9)), (3, [12, 13, 13] + up(14, 6))],
             noN=4, noC=33, noCA=12, unk=40),
        dict(pep=(30, 5), frags=[(2, up(-20, 30)), (1, up(1500, 2))], noN=11, noC=22, noCA=27, unk=36),
        None,                                                                                         # a fully padded sample
    ]),
    "long130": (130, 3501, [
        dict(pep=(60, 12), frags=[(1, up(1, 40)), (1, up(42, 20)), (2, up(1100, 30)), (3, down(-5, 28))], noN=50, noC=100, noCA=25, unk=110),
    ]),
    # frag19's first topology, other geometry; `pair`: (i, j) with C_i, N_j, CA_j collinear, `omega`: k with CA_k, C_k, N_k+1 collinear
    "collinear": (19, 3601, [
        dict(pep=(7, 5), frags=[(1, up(1043, 4)), (1, up(1048, 3)), (2, down(-3, 4)), (2, [57, 57, 58])], noN=2, noC=17, noCA=16, unk=5,
             pair=(6, 13), omega=0),
    ]),
}
CASES = tuple(_SPECS) + ("collinear_garbage",)
F16_CASES = ("frag19", "frag33", "wrap40", "collinear")        # what golden F16 holds the reference's outputs for
SWITCHES = ((True, True), (True, False), (False, True), (False, False))      # (sample_structure, sample_sequence)


def dihedral_terms(p0, p1, p2, p3):
    """(u1, sign) of dihedral_from_four_points (geometry.py:296-313) in torch fp32: what decides whether the clamp sees a NaN."""
    p0, p1, p2, p3 = (torch.as_tensor(np.asarray(p, dtype=np.float32)) for p in (p0, p1, p2, p3))
    v0, v1, v2 = p2 - p1, p0 - p1, p3 - p2
    return torch.linalg.cross(v0, v1, dim=-1), torch.sign((torch.linalg.cross(v1, v2, dim=-1) * v0).sum(-1))


def _frame_margins(p):
    """min over the residues that have N, CA or C of (|C - CA|, |component of N - CA orthogonal to C - CA|), float64."""
    pos, msk = p["pos_heavyatom"].astype(np.float64), p["mask_heavyatom"]
    has = msk[:, :3].any(-1)
    v1 = pos[:, BB_C] - pos[:, BB_CA]
    n1 = np.linalg.norm(v1, axis=-1)
    e1 = v1 / np.maximum(n1, 1e-30)[:, None]
    v2 = pos[:, BB_N] - pos[:, BB_CA]
    n2 = np.linalg.norm(v2 - (e1 * v2).sum(-1, keepdims=True) * e1, axis=-1)
    return (float(n1[has].min()), float(n2[has].min())) if has.any() else (np.inf, np.inf)


def _drop_atom(p, r, slot):
    p["mask_heavyatom"][r, slot] = False
    p["pos_heavyatom"][r, slot] = 0.0


def _grid(x):
    return np.round(np.asarray(x, dtype=np.float64) * 4.0) / 4.0          # multiples of 1/4 A: differences of such points are exact in fp32


def _place_collinear(p, spec):
    """The issue's construction (p1 = G, p2 = G + v0, p0 = G + 2 v0, p3 = p2 + randn(3)) on the backbone, twice:
    EdgeEmbedder's phi of the pair (i, j): dih(C_i, N_j, CA_j, C_j); NodeEmbedder's omega of k + 1: dih(CA_k, C_k, N_k+1, CA_k+1).
    The draws come from torch.Generator().manual_seed(0) in order; a draw is taken when u1 == 0 exactly, the sign of the triple
    product is not 0 and the frames stay conditioned.  -> the two point quadruples [2, 4, 3]."""
    pos = p["pos_heavyatom"]
    v0 = np.asarray(COLLINEAR_V0, dtype=np.float64)
    gen = torch.Generator().manual_seed(0)
    (i, j), k = spec["pair"], spec["omega"]
    out = []
    for which in ("pair", "omega"):
        g = _grid(pos[j, BB_N] if which == "pair" else pos[k, BB_C])
        for _ in range(64):
            r = torch.randn(3, generator=gen).numpy().astype(np.float64)
            trial = pos.copy()
            if which == "pair":
                trial[j, BB_N], trial[j, BB_CA], trial[i, BB_C] = g, g + v0, g + 2 * v0
                trial[j, BB_C] = (trial[j, BB_CA].astype(np.float32) + r.astype(np.float32))
                quad = trial[[i, j, j, j], [BB_C, BB_N, BB_CA, BB_C]]
            else:
                trial[k, BB_C], trial[k + 1, BB_N], trial[k, BB_CA] = g, g + v0, g + 2 * v0
                trial[k + 1, BB_CA] = (trial[k + 1, BB_N].astype(np.float32) + r.astype(np.float32))
                quad = trial[[k, k, k + 1, k + 1], [BB_CA, BB_C, BB_N, BB_CA]]
            u1, sgn = dihedral_terms(*quad)
            q = dict(p, pos_heavyatom=trial)
            if bool((u1 == 0).all()) and float(sgn) != 0.0 and min(_frame_margins(q)) > 0.5:
                pos[:] = trial
                out.append(quad.copy())
                break
        else:
            raise AssertionError(f"no draw gives the degenerate {which} dihedral")
    return np.stack(out)


def _sample(rng, spec, seed):
    first, n_gen = spec["pep"]
    n_ctx = sum(len(nb) for _, nb in spec["frags"])
    n = n_ctx + n_gen
    p = synth.make_pocket(np.random.Generator(np.random.PCG64(seed)), n_ctx, n_gen)
    order = list(range(first)) + list(range(n_ctx, n)) + list(range(first, n_ctx))     # peptide moved into the middle
    p = {k: np.ascontiguousarray(v[order]) for k, v in p.items()}
    chain, nb = [c for c, f in spec["frags"] for _ in f], [x for _, f in spec["frags"] for x in f]
    p["chain_nb"] = np.array(chain[:first] + [0] * n_gen + chain[first:], dtype=np.int64)
    p["res_nb"] = np.array(nb[:first] + up(1, n_gen) + nb[first:], dtype=np.int64)
    gen = p["generate_mask"]
    assert gen[first:first + n_gen].all() and gen.sum() == n_gen and not gen[0] and not gen[-1]
    # random missing side-chain atoms (slots 4..: CB and beyond), context and peptide alike
    drop = (rng.random(p["mask_heavyatom"].shape) < 0.15) & p["mask_heavyatom"]
    drop[:, :4] = False
    p["mask_heavyatom"] &= ~drop
    edited = [spec[k] for k in ("noN", "noC", "noCA", "unk")]
    assert len(set(edited)) == 4 and not gen[edited].any()
    _drop_atom(p, spec["noN"], BB_N)
    _drop_atom(p, spec["noC"], BB_C)
    _drop_atom(p, spec["noCA"], BB_CA)
    p["aa"][spec["unk"]] = UNK_AA
    p["pos_heavyatom"][~p["mask_heavyatom"]] = 0.0
    if "pair" in spec:
        touched = {spec["pair"][0], spec["pair"][1], spec["omega"], spec["omega"] + 1}
        assert len(touched) == 4 and not (touched & set(edited)) and not gen[list(touched)].any()
        p["collinear_points"] = _place_collinear(p, spec)
    m = _frame_margins(p)
    assert min(m) > 0.5, ("ill-conditioned frame", m)
    return p


def _pad(v, L, key):
    fill = PAD_AA if key == "aa" else 0
    out = np.full((L,) + v.shape[1:], fill, dtype=v.dtype)
    out[:v.shape[0]] = v
    return out


def make(name):
    """-> batch dict of CPU tensors (PaddingCollate schema, pepflow/utils/data.py:63-78) of the named case.  `collinear` and
    `collinear_garbage` also carry 'collinear_points' [2, 4, 3]: the (p0, p1, p2, p3) of the two degenerate dihedrals."""
    garbage = name == "collinear_garbage"
    L, seed, specs = _SPECS["collinear" if garbage else name]
    rng = np.random.Generator(np.random.PCG64(seed))
    items = [(_sample(rng, s, seed + 7 * b) if s is not None else None) for b, s in enumerate(specs)]
    keys = [k for k in next(it for it in items if it is not None) if k != "collinear_points"]
    like = next(it for it in items if it is not None)
    out = {}
    for k in keys:
        rows = [_pad(it[k] if it is not None else like[k][:0], L, k) for it in items]
        out[k] = torch.from_numpy(np.stack(rows))
    lengths = [0 if it is None else len(it["aa"]) for it in items]
    out["res_mask"] = torch.stack([torch.arange(L) < n for n in lengths])
    assert max(lengths) == L
    if "collinear_points" in items[0]:
        out["collinear_points"] = torch.from_numpy(items[0]["collinear_points"].astype(np.float32))
    return garbage_in_masked_sidechains(out, seed + 1) if garbage else out


def garbage_in_masked_sidechains(batch, seed=11):
    """The batch with finite garbage (|x| up to 1e3) in the positions of masked non-backbone atoms of real residues."""
    g = np.random.Generator(np.random.PCG64(seed)).uniform(-1e3, 1e3, size=tuple(batch["pos_heavyatom"].shape)).astype(np.float32)
    hole = ~batch["mask_heavyatom"].numpy()
    hole[:, :, :3] = False
    hole &= batch["res_mask"].numpy()[:, :, None]
    assert hole.any()
    return dict(batch, pos_heavyatom=torch.from_numpy(np.where(hole[..., None], g, batch["pos_heavyatom"].numpy())))


def model_inputs(batch):
    """What model.encode / O.encode take (without the case's bookkeeping arrays)."""
    return {k: v for k, v in batch.items() if k != "collinear_points"}


def coverage(batch):
    """What a batch drives, from its arrays alone (asserted by the CPU test so that an edit of a spec cannot silently lose a branch)."""
    rm, gen = batch["res_mask"], batch["generate_mask"]
    nb, ch = batch["res_nb"], batch["chain_nb"]
    real2 = rm[:, :, None] & rm[:, None, :]
    d = (nb[:, :, None] - nb[:, None, :])[real2 & (ch[:, :, None] == ch[:, None, :])]
    step = (nb[:, 1:] - nb[:, :-1])[rm[:, 1:] & rm[:, :-1] & (ch[:, 1:] == ch[:, :-1])]
    cross = (nb[:, :, None] == nb[:, None, :]) & (ch[:, :, None] != ch[:, None, :]) & real2
    m = batch["mask_heavyatom"]
    ctx = m[:, :, BB_CA] & ~gen
    return {
        "chains": sorted(set(ch[rm].tolist())), "max_res_nb": int(nb[rm].max()) if rm.any() else 0, "min_res_nb": int(nb[rm].min()) if rm.any() else 0,
        "steps": sorted(set(step.tolist())), "relpos_rows": sorted(set((d.clamp(-32, 32) + 32).tolist())),
        "beyond_clamp": bool((d > 32).any() and (d < -32).any()), "same_number_other_chain": bool(cross.any()),
        "no_N": int((rm & ~m[:, :, BB_N] & m[:, :, BB_CA] & ~gen).sum()), "no_C": int((rm & ~m[:, :, BB_C] & m[:, :, BB_CA] & ~gen).sum()),
        "no_CA": int((rm & ~m[:, :, BB_CA] & m[:, :, BB_N] & m[:, :, BB_C]).sum()),
        "unk_context": int((ctx & (batch["aa"] == UNK_AA)).sum()), "peptide_lengths": gen.sum(1).tolist(),
        "lengths": rm.sum(1).tolist(), "context_at_both_ends": [bool(n and ctx[b, 0] and ctx[b, n - 1]) for b, n in enumerate(rm.sum(1).tolist())],
    }


# ---- golden F16 (tests/golden/make_golden_f16.py): the reference's encode() on F16_CASES ------------------------------------------
def load_f16(golden_dir):
    """Both F16 files as one dict of tensors, keys '<case>.<array>'."""
    out = {}
    for name in ("f16_encode_inputs.npz", "f16_encode_edges.npz"):
        d = np.load(os.path.join(golden_dir, name))
        out.update({k: torch.from_numpy(d[k]) for k in d.files})
    return out


def f16_batch(f16, case):
    pfx = case + ".batch_"
    return {k[len(pfx):]: v for k, v in f16.items() if k.startswith(pfx)}
