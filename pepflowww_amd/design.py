"""De novo design entry: from a bare receptor structure to a batch that `FlowModel.sample` accepts, with no native peptide anywhere.

  receptor_from_pdb(path, chains=None)   -> the receptor's per-residue dict (`preprocess.parse_pdb` + `get_torsion_angle`);
  find_cavities(receptor, ...)           -> candidate binding sites: `geometry.cavity_scan` (pf_cavity_fwd, on the device) over the
                                            grid of `geometry.cavity_grid`, one entry per cavity, in the receptor's own coordinates;
  make_design_batch(receptor, length, n_samples, cavity= | center= | hotspots=)
                                         -> (batch, info): the context residues around the site, centred on it, followed by `length`
                                            placeholder peptide rows, with the conventions of `preprocess.preprocess_structure` and
                                            the padding of `io.PaddingCollate`;
  to_receptor_frame(x, info)             -> sampled coordinates back in the receptor's frame.

Why placeholders are enough: every generated row of sample()'s state starts from noise, and the embedders mask the generated rows'
coordinates and residue types (the reference's flow_model.py:85-91, `structure_mask` / `sequence_mask` in node.py and edge.py), so the
values in the placeholder rows do not reach the trajectory; tests/test_gpu_design.py holds that bit for bit.

Caveats ("De novo design entry"): the scan follows the LIGSITE publication (Hendlich et al. 1997) and is not checked
against that program or fpocket; its defaults are untuned; the training pockets were cut around native peptides by a rule the
reference does not state, so a geometric cut is an off-label input.  Host code apart from the scan."""
import torch

from . import geometry
from .io import PaddingCollate
from .preprocess import CA, UNK, get_torsion_angle, parse_pdb

MAX_RESIDUES = 512                      # context + peptide rows of one sample (the evaluation kernels' bound)
_PER_RESIDUE = ("chain_id", "chain_nb", "resseq", "icode", "res_nb", "aa", "pos_heavyatom", "mask_heavyatom")


def receptor_from_pdb(path, chains=None):
    """The receptor of a PDB file as parse_pdb's per-residue dict (chain_id, chain_nb, resseq, icode, res_nb, aa, pos_heavyatom
    [N,15,3], mask_heavyatom [N,15]) plus torsion_angle / torsion_angle_mask [N,5] in the file's own frame.  chains: the chain
    identifiers to keep (None: all)."""
    data, _ = parse_pdb(path)
    if data is None:
        raise ValueError(f"{path}: no amino-acid residues found")
    if chains is not None:
        chains = set(chains)
        keep = [i for i, c in enumerate(data["chain_id"]) if c in chains]
        if not keep:
            raise ValueError(f"{path}: no residues in chains {sorted(chains)}; the file has {sorted(set(data['chain_id']))}")
        data = _rows(data, keep)
    data["torsion_angle"], data["torsion_angle_mask"] = get_torsion_angle(data["pos_heavyatom"], data["aa"])
    return data


def _rows(data, idx):
    """the residues `idx` (a list) of a per-residue dict"""
    sel = torch.as_tensor(idx, dtype=torch.int64)
    return {k: (v[sel] if isinstance(v, torch.Tensor) else [v[i] for i in idx]) for k, v in data.items()}


def find_cavities(receptor, h=1.0, margin=8.0, device="cuda", **scan_params):
    """Candidate binding sites of a receptor (receptor_from_pdb's dict, or any dict with aa [N], pos_heavyatom [N,15,3] and
    mask_heavyatom [N,15]): builds the grid (`geometry.cavity_grid`), runs `geometry.cavity_scan` on `device` and reads the result
    back.  scan_params: geometry.CAVITY_DEFAULTS.
    -> list, best rank first, of dicts: rank, size (points), volume = size * h^3 (A^3), center [3], mean_buried, lining (int64
    indices of the lining residues), points [size,3] (the member points) -- coordinates in the receptor's own frame -- and h."""
    pos, mask, aa = receptor["pos_heavyatom"][None], receptor["mask_heavyatom"][None], receptor["aa"][None]
    origin, dims = geometry.cavity_grid(pos, mask, h=h, margin=margin)
    out = geometry.cavity_scan(pos.to(device), mask.to(device), aa.to(device), origin.to(device), dims, h=h, **scan_params)
    geometry.cavity_check(out["status"])
    n = min(int(out["n_found"][0]), out["size"].shape[1])
    label = out["label"][0].cpu().reshape(dims)
    size, center, buried, lining = (out[k][0].cpu() for k in ("size", "center", "mean_buried", "lining"))
    res = []
    for k in range(n):
        ijk = (label == k).nonzero().to(torch.float32)                                  # in linear-index order
        res.append({"rank": k, "size": int(size[k]), "volume": int(size[k]) * float(h) ** 3, "center": center[k].clone(),
                    "mean_buried": float(buried[k]), "lining": lining[k].nonzero().flatten(),
                    "points": origin[0][None, :] + ijk * torch.tensor(float(h), dtype=torch.float32), "h": float(h)})
    return res


def _site(receptor, cavity, center, hotspots):
    """-> (kind, centre [3] float32, the site's points [P,3] float32, hot-spot residue indices of the receptor or None)"""
    given = [k for k, v in (("cavity", cavity), ("center", center), ("hotspots", hotspots)) if v is not None]
    if len(given) != 1:
        raise ValueError(f"exactly one of cavity=, center=, hotspots= chooses the site, got {given or 'none'}")
    N = receptor["aa"].shape[0]
    if cavity is not None:
        if not isinstance(cavity, dict) or not {"center", "points", "lining"} <= set(cavity):
            raise ValueError("cavity must be an entry of find_cavities")
        return "cavity", cavity["center"].to(torch.float32), cavity["points"].to(torch.float32), cavity["lining"].to(torch.int64)
    if center is not None:
        c = torch.as_tensor(center, dtype=torch.float32)
        if tuple(c.shape) != (3,) or not bool(torch.isfinite(c).all()):
            raise ValueError(f"center must be three finite coordinates, got {center!r}")
        return "center", c, c[None], None
    hot = torch.as_tensor(hotspots, dtype=torch.int64).flatten()
    if hot.numel() == 0 or int(hot.min()) < 0 or int(hot.max()) >= N or hot.unique().numel() != hot.numel():
        raise ValueError(f"hotspots must be distinct receptor residue indices in 0..{N - 1}, got {hotspots!r}")
    if not bool(receptor["mask_heavyatom"][hot, CA].all()):
        raise ValueError("every hot-spot residue needs its CA atom")
    c = receptor["pos_heavyatom"][hot, CA].to(torch.float32).mean(0)
    return "hotspots", c, c[None], hot


def _context(receptor, points, radius, max_context):
    """receptor residues with an atom (mask set) within `radius` of one of `points`; at most max_context, the nearest first (ties by
    index); -> their indices in receptor order"""
    pos, mask = receptor["pos_heavyatom"].to(torch.float32), receptor["mask_heavyatom"].bool()
    N, A = mask.shape
    near = torch.full((N,), float("inf"))
    flat = pos.reshape(N * A, 3)
    for p0 in range(0, points.shape[0], 1024):                                          # [N * A, <= 1024] at a time
        d = torch.cdist(flat, points[p0:p0 + 1024], compute_mode="donot_use_mm_for_euclid_dist").min(1).values.reshape(N, A)
        near = torch.minimum(near, d.masked_fill(~mask, float("inf")).min(1).values)
    idx = (near <= radius).nonzero().flatten()
    if idx.numel() > max_context:
        order = sorted(idx.tolist(), key=lambda i: (float(near[i]), i))[:max_context]
        idx = torch.tensor(sorted(order), dtype=torch.int64)
    return idx


def make_design_batch(receptor, length, n_samples, *, cavity=None, center=None, hotspots=None, radius=10.0, max_context=None):
    """A batch for `FlowModel.sample` that designs a peptide of `length` residues at a site of the receptor, n_samples times.

    Exactly one of cavity (an entry of find_cavities), center (a point, receptor frame) and hotspots (receptor residue indices: the
    site is their CA centroid) chooses the site.  Context: the receptor residues with an atom within `radius` of the site's points
    (the cavity's member points, or the one point), at most max_context (default 512 - length), the nearest first, ties by index,
    kept in receptor order.  Coordinates are shifted so that the site's centre is the origin (sample()'s initial translation noise is
    zero-centred there); torsions are computed after the shift, as preprocess_structure does.  `length` placeholder rows follow:
    chain_nb 0 (the receptor's + 1), res_nb 1..length, generate_mask, backbone atoms (N, CA, C, O) in mask_heavyatom, zero
    coordinates, aa = UNK, zero torsions, torsion_angle_mask true for psi only.  Padding as PaddingCollate.
    -> (batch, info): batch has preprocess_structure's keys (+ res_mask), every sample the same; info = {center [3], context_index
    (into the receptor), hotspots (bool [L]: the cavity's lining residues or the given hot spots, in batch numbering, ready for
    guide=), site (which argument chose it), length}."""
    for name, v in (("length", length), ("n_samples", n_samples)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if length >= MAX_RESIDUES:
        raise ValueError(f"length must be below {MAX_RESIDUES}, got {length}")
    if max_context is None:
        max_context = MAX_RESIDUES - length
    if not isinstance(max_context, int) or isinstance(max_context, bool) or not 1 <= max_context <= MAX_RESIDUES - length:
        raise ValueError(f"max_context must be in 1..{MAX_RESIDUES - length}, got {max_context!r}")
    radius = float(radius)
    if not 0.0 < radius < float("inf"):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    kind, c, points, hot = _site(receptor, cavity, center, hotspots)
    idx = _context(receptor, points, radius, max_context)
    if idx.numel() == 0:
        raise ValueError(f"no receptor residue within {radius} A of the site")
    rec = _rows({k: receptor[k] for k in _PER_RESIDUE}, idx.tolist())
    rec["pos_heavyatom"] = rec["pos_heavyatom"].to(torch.float32) - c[None, None, :]
    rec["torsion_angle"], rec["torsion_angle_mask"] = get_torsion_angle(rec["pos_heavyatom"], rec["aa"])
    rec["chain_nb"] = rec["chain_nb"] + 1
    used = set(rec["chain_id"])
    pep_chain = next(ch for ch in "PQRSTUVWXYZABCDEFGHIJKLMNOpqrstuvwxyz0123456789" if ch not in used)
    bb = torch.zeros(length, 15, dtype=torch.bool)
    bb[:, :4] = True
    tmask = torch.zeros(length, 5, dtype=torch.bool)
    tmask[:, 0] = True
    pep = {"chain_id": [pep_chain] * length, "chain_nb": torch.zeros(length, dtype=torch.int64),
           "resseq": torch.arange(1, length + 1), "icode": [" "] * length, "res_nb": torch.arange(1, length + 1),
           "aa": torch.full((length,), UNK, dtype=torch.int64), "pos_heavyatom": torch.zeros(length, 15, 3), "mask_heavyatom": bb,
           "torsion_angle": torch.zeros(length, 5), "torsion_angle_mask": tmask}
    n_ctx = idx.numel()
    sample = {"id": f"design_{kind}",
              "generate_mask": torch.cat([torch.zeros(n_ctx, dtype=torch.bool), torch.ones(length, dtype=torch.bool)])}
    for k, v in rec.items():
        sample[k] = torch.cat([v, pep[k]], 0) if isinstance(v, torch.Tensor) else v + pep[k]
    batch = PaddingCollate()([sample] * n_samples)
    L = batch["aa"].shape[1]
    hot_rows = torch.zeros(L, dtype=torch.bool)
    if hot is not None:
        where = {int(r): j for j, r in enumerate(idx.tolist())}
        for r in hot.tolist():
            if r in where:
                hot_rows[where[r]] = True
    info = {"center": c.clone(), "context_index": idx, "hotspots": hot_rows, "site": kind, "length": length}
    return batch, info


def batch_to(batch, device):
    """the batch with its tensors on `device` (the lists of chain identifiers and insertion codes stay as they are)"""
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}


def to_receptor_frame(x, info):
    """coordinates [..., 3] of the batch's frame (sample()'s trans_*, reconstructed atoms) back in the receptor's own frame"""
    return x + info["center"].to(x)
