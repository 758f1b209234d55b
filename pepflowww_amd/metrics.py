"""Quality metrics of sampled peptides on the device: what the reference's sampling driver reports after `sample()`
(models_con/inference.py:77-79: CA RMSD, rotation RMSD, amino-acid recovery) and what its evaluation adds (eval/geometry.py:
CA RMSD after superposition, `get_rmsd` 47-59; binding-site ratio, `get_bind_site` / `get_bind_ratio` 93-110; diversity among the
samples of one complex), without Biopython / tmtools / mdtraj and without writing PDB files; TM-score against the native, novelty
and TM-score diversity (`structure_scores`); DSSP secondary structure and the secondary-structure ratio, `get_second_stru` / `get_ss`
79-91 (`secondary_structure`); clashes and broken peptide bonds, AlphaFold's between-residue structural violations
(`structural_violations`); solvent-accessible surface and the area buried between peptide and receptor (`interface_area`); the
side-chain packing table, chi1-chi4 errors against the native and the share of residues with every chi within a tolerance
(`sidechain_packing`); superposition-free local accuracy, lDDT with the values of OpenFold's lddt / lddt_ca
(openfold/utils/loss.py:382-458), over the peptide and across the interface (`local_accuracy`); docking quality, Fnat, iRMSD, LRMSD and
DockQ (`docking_quality`); an empirical peptide-receptor interface energy, the functional form of AutoDock Vina's scoring function
written from the publication and not checked against that program (`binding_energy`); directional hydrogen bonds and salt bridges
across the interface and the buried polar atoms without a hydrogen-bond partner, heavy-atom criteria written from the publications and
not checked against HBPLUS, PLIP or Rosetta (`polar_satisfaction`); structural clusters of the samples of each
complex, their representatives and the best-scored member of each (`cluster_samples`: gromos clustering after Daura et al. 1999, which
follows the publication and is not checked against GROMACS, and single / complete / average linkage cut at a height, checked against
scipy's fcluster(criterion="distance") as partitions only); rotamer side chains for a backbone-only sample, a staggered rotamer grid
scored with the interface energy's pair function and chosen by iterated conditional modes, which is not SCWRL4 and not Rosetta's
packer and takes their place in role only (`pack_samples`, and backbone="packed" in the structure metrics); point-mutation scanning of
the generated residues, an alanine scan and a position scan with the packer's self energy on an unmoved environment, which is not FoldX
(eval/foldx.py) and not Rosetta and takes their place in role only (`mutation_scan`); the reference's `diff_ratio` (difflib's SequenceMatcher ratio, exact values), an
alignment identity across lengths and the nearest known sequence of a library (`sequence_scores`).

Every per-residue, per-point and per-atom-pair operation runs in pf_superpose_fwd / pf_binding_site_fwd / pf_tm_score_fwd / pf_dssp_fwd /
pf_violations_fwd / pf_sasa_fwd / pf_torsions_fwd / pf_sidechain_compare_fwd / pf_lddt_fwd / pf_contacts_fwd / pf_interface_energy_fwd / pf_polar_fwd / pf_relax_fwd / pf_cluster_fwd / pf_pack_sidechains_fwd / pf_mutation_scan_fwd / pf_sequence_design_fwd / pf_seq_ratio_fwd / pf_seq_align_fwd / pf_seq_search_fwd (and the backbone reconstruction kernels); the host builds pair lists and masks and combines per-sample (or per-pair) outputs."""
import ctypes as C
import math

import torch

from . import _capi, full_atom
from . import geometry
from .geometry import dssp, group_pairs, ss_simplify, superpose, tm_align, tm_score

BIND_CUTOFF = 10.0          # eval/geometry.py:100: receptor residues within 10 A of a peptide CA
CA_ATOM = 1                 # BBHeavyAtom.CA


def _check_groups(gen, groups):
    """-> group labels [B] (CPU int64).  The samples of one group must share the generate mask (one complex, replicated)."""
    B = gen.shape[0]
    g = torch.zeros(B, dtype=torch.int64) if groups is None else torch.as_tensor(groups).reshape(-1).cpu().to(torch.int64)
    if g.numel() != B:
        raise ValueError(f"groups has {g.numel()} labels for {B} samples")
    gen = gen.cpu().bool()
    for lab in torch.unique(g):
        rows = gen[g == lab]
        if not bool((rows == rows[0]).all()):
            raise ValueError("samples of one group must have the same generate_mask"
                             + (" (groups=None treats the batch as one complex; pass groups for a batch of several)" if groups is None else ""))
    return g


def _device(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _group_sum(values, index, G, dtype=torch.float64):
    """values [n, ...] summed into G rows by index [n]; a mean is the quotient of two of these (0 / 0: NaN for an empty group)"""
    return torch.zeros((G,) + tuple(values.shape[1:]), dtype=dtype, device=values.device).index_add_(0, index, values.to(dtype))


def _check_backbone(backbone):
    if backbone not in ("full_atom", "frames", "packed"):
        raise ValueError(f"backbone must be 'full_atom', 'frames' or 'packed', got {backbone!r}")


def _complexes(final, batch, backbone="full_atom", index=False):
    """The two complexes the structure metrics compare.  The sample: generated residues rebuilt from the final state -- backbone
    "full_atom": all heavy atoms (reconstruct_sample: rotmats, trans, angles, seqs), "frames": N, CA, C, O (reconstruct_sample_bb),
    "packed": the "frames" complex with the generated residues' side chains placed by geometry.pack_sidechains with its defaults (a
    staggered rotamer grid and the package's own pair energy; not SCWRL4, whose place it takes in role only) -- with the context
    kept, types where(generate, seqs, seqs_1).  The native: pos_heavyatom / mask_heavyatom / seqs_1.
    `backbone` is checked before final / batch are touched.
    -> (device, res_mask, gen = generate_mask & res_mask, `residue_index` of the batch if `index` else None,
        (pos_s, mask_s, aa_s), (pos_n, mask_n, seqs_1))"""
    _check_backbone(backbone)
    dev = _device(batch["generate_mask"], final["trans"], batch["pos_heavyatom"])
    res_mask = batch["res_mask"].to(dev).bool()
    gen = batch["generate_mask"].to(dev).bool() & res_mask
    rotmats, trans, seqs, seqs_1 = (final[k].to(dev) for k in ("rotmats", "trans", "seqs", "seqs_1"))
    pos_n, mask_n = batch["pos_heavyatom"].to(dev), batch["mask_heavyatom"].to(dev).bool()
    if backbone == "full_atom":
        pos_s, mask_s = full_atom.reconstruct_sample(rotmats, trans, final["angles"].to(dev), seqs, gen, pos_n)
        mask_s = torch.where(gen[:, :, None], mask_s, mask_n[:, :, :15])
    else:
        pos_s, mask_s = full_atom.reconstruct_sample_bb(rotmats, trans, seqs, batch["chain_nb"].to(dev), batch["res_nb"].to(dev),
                                                        res_mask, gen, pos_n, mask_n)
    packed = backbone == "packed"
    idx = residue_index(batch["chain_nb"].to(dev), batch["res_nb"].to(dev), res_mask) if index or packed else None
    aa_s = torch.where(gen, seqs, seqs_1)
    if packed:
        p = geometry.pack_sidechains(pos_s, mask_s & res_mask[:, :, None], aa_s, idx, gen)
        pos_s, mask_s = p["pos"], torch.where(p["packed"][:, :, None], p["atom_mask"], mask_s)
    return dev, res_mask, gen, idx if index else None, (pos_s, mask_s, aa_s), (pos_n, mask_n, seqs_1)


def binding_site(ctx_pos, ctx_atom_mask, res_mask, gen_mask, pep_sample, pep_native, cutoff=BIND_CUTOFF, ca_atom=CA_ATOM):
    """pf_binding_site_fwd -> (site_sample [B,L] bool, site_native [B,L] bool, bsr [B])."""
    B, L, A, _ = ctx_pos.shape
    dev = _device(ctx_pos, pep_sample, res_mask)
    keep = [ctx_pos.to(dev, torch.float32).contiguous(), ctx_atom_mask.to(dev).to(torch.uint8).contiguous(),
            res_mask.to(dev).to(torch.uint8).contiguous(), gen_mask.to(dev).to(torch.uint8).contiguous(),
            pep_sample.to(dev, torch.float32).reshape(B, L, 3).contiguous(), pep_native.to(dev, torch.float32).reshape(B, L, 3).contiguous()]
    s_site, n_site = torch.empty(B, L, dtype=torch.uint8, device=dev), torch.empty(B, L, dtype=torch.uint8, device=dev)
    bsr = torch.empty(B, device=dev)
    a = _capi.BindingSiteArgs()
    a.ctx_pos, a.ctx_atom_mask, a.res_mask, a.gen_mask, a.pep_sample, a.pep_native = (
        _capi.dptr(t, t.dtype, "binding_site input") for t in keep)
    a.n_atoms, a.ca_atom, a.cutoff, a.B, a.L = A, ca_atom, float(cutoff), B, L
    a.site_sample, a.site_native, a.bsr = s_site.data_ptr(), n_site.data_ptr(), bsr.data_ptr()
    _capi.check(_capi.load().pf_binding_site_fwd(C.byref(a), _capi.stream_ptr()), "pf_binding_site_fwd")
    return s_site.bool(), n_site.bool(), bsr


def evaluate_samples(final, batch, groups=None):
    """final: traj[-1] of FlowModel.sample (keys rotmats, trans, seqs, rotmats_1, trans_1, seqs_1; CPU or device tensors);
    batch: generate_mask, res_mask, pos_heavyatom, mask_heavyatom.  groups [B]: the complex of each sample (None: one complex,
    which needs the same generate_mask in every sample; ValueError otherwise).

    -> dict of device tensors.  Per sample [B], over the generated residues:
      ca_rmsd          RMSD of trans against trans_1, no superposition;
      ca_rmsd_aligned  the same after the optimal proper superposition (get_rmsd's second value);
      rot_rmsd         sqrt(sum ||R - R_1||_F^2 / n): sqrt(3) x the plain RMSD of the matrix rows taken as three points per residue;
      aar              fraction of seqs equal to seqs_1;
      bsr              binding-site ratio: receptor residues within 10 A of a sampled peptide CA that are also within 10 A of a
                       native one, over the latter (+1e-10);
      count            generated residues; site_sample / site_native [B,L] the two binding sites.
    Pooled over the batch (float64 scalars), inference.py:77-79 with their +1e-8: ca_rmsd_pooled, rot_rmsd_pooled, aar_pooled.
    Per group [G] (labels in group_labels): diversity_rmsd = mean aligned CA RMSD over the pairs i < j, diversity_seq = 1 - their
    mean sequence identity (NaN for a group of one)."""
    gen_cpu = batch["generate_mask"]
    labels = _check_groups(gen_cpu, groups)
    dev = _device(batch["generate_mask"], final["trans"], batch["pos_heavyatom"])
    final = {k: final[k].to(dev) for k in ("rotmats", "trans", "seqs", "rotmats_1", "trans_1", "seqs_1")}
    B, L = final["seqs"].shape
    gen = batch["generate_mask"].to(dev).bool()
    ids = torch.arange(B, dtype=torch.int32)
    diag = torch.stack([ids, ids], 1)

    ca = superpose(final["trans"], final["trans_1"], gen, gen, diag, aa_x=final["seqs"], aa_y=final["seqs_1"])
    gen3 = gen[:, :, None].expand(B, L, 3).reshape(B, 3 * L)
    # ||R - R_1||_F^2 is the summed squared distance of the three rows (equally: the three columns) taken as points
    rot = superpose(final["rotmats"].reshape(B, 3 * L, 3), final["rotmats_1"].reshape(B, 3 * L, 3), gen3, gen3, diag)

    pairs, gidx, glab = group_pairs(labels)
    div = superpose(final["trans"], final["trans"], gen, gen, pairs, aa_x=final["seqs"], aa_y=final["seqs"])
    G = glab.numel()
    gidx = gidx.to(dev)
    npair = _group_sum(torch.ones_like(gidx), gidx, G)
    div_rmsd = _group_sum(div["rmsd"], gidx, G) / npair
    div_seq = 1.0 - _group_sum(div["ident"], gidx, G) / npair

    s_site, n_site, bsr = binding_site(batch["pos_heavyatom"], batch["mask_heavyatom"], batch["res_mask"], gen, final["trans"],
                                       final["trans_1"])

    n = ca["count"].double()
    rot_rmsd = rot["rmsd_plain"] * math.sqrt(3.0)
    tot = n.sum() + 1e-8
    # per-sample sums back from the per-sample means (samples without generated residues contribute nothing)
    ca_sum = torch.nan_to_num(ca["rmsd_plain"].double() ** 2 * n).sum()
    rot_sum = torch.nan_to_num(rot["rmsd_plain"].double() ** 2 * 3.0 * n).sum()
    same = torch.nan_to_num(torch.round(ca["ident"].double() * n)).sum()
    return {"ca_rmsd": ca["rmsd_plain"], "ca_rmsd_aligned": ca["rmsd"], "rot_rmsd": rot_rmsd, "aar": ca["ident"], "bsr": bsr,
            "count": ca["count"], "site_sample": s_site, "site_native": n_site,
            "ca_rmsd_pooled": torch.sqrt(ca_sum / tot), "rot_rmsd_pooled": torch.sqrt(rot_sum / tot), "aar_pooled": same / tot,
            "diversity_rmsd": div_rmsd, "diversity_seq": div_seq, "group_labels": glab.to(dev)}


def structure_scores(final, batch, groups=None, novelty_tm=0.5, novelty_ident=0.5, tm_mode="fixed"):
    """TM-score of the sampled CAs (`trans`) against the native ones (`trans_1`) over the generated residues, and two combinations
    of it.  final / batch / groups as in `evaluate_samples` (only final["trans"], ["trans_1"], ["seqs"], ["seqs_1"] and
    batch["generate_mask"] are read).  The TM-score keeps the residue correspondence fixed (the TMscore program's search, not
    TM-align's), normalised by the native's generated count (tmtools' tm_norm_chain2).

    -> dict of device tensors:
      tm           [B] sample onto native (NaN below 3 generated residues);
      tm_pooled    mean of tm (float64 scalar);
      novel        [B] bool: tm < novelty_tm and aar < novelty_ident, aar = positional sequence identity to seqs_1 (the fraction of
                   generated positions with the same residue type; not the reference's difflib ratio);
      novelty      [G] fraction of novel samples in each group;
      diversity_tm [G] 1 - mean TM-score over the pairs i < j of the group (sample i onto sample j), NaN for a group of one;
      group_labels [G].
    `novel`, `novelty` and `diversity_tm` are this package's definitions, with thresholds of the caller's choosing.

    tm_mode: "fixed" (the default) -- the fixed-correspondence TM-score above; "tmalign" -- TM-align (geometry.tm_align): tm is the
    sample aligned onto the native normalised by the native's length (tmtools' tm_norm_chain2, what eval/geometry.py's get_tm
    returns), and novel, novelty and diversity_tm (sample i aligned onto sample j) use it.  The keys are the same in both modes."""
    if tm_mode not in ("fixed", "tmalign"):
        raise ValueError(f"tm_mode must be 'fixed' or 'tmalign', got {tm_mode!r}")
    labels = _check_groups(batch["generate_mask"], groups)
    dev = _device(batch["generate_mask"], final["trans"])
    final = {k: final[k].to(dev) for k in ("trans", "seqs", "trans_1", "seqs_1")}
    B = final["seqs"].shape[0]
    gen = batch["generate_mask"].to(dev).bool()
    ids = torch.arange(B, dtype=torch.int32)
    diag = torch.stack([ids, ids], 1)

    if tm_mode == "tmalign":
        max_len = int(gen.sum(1).max()) if B else 0
        score = lambda x, y, pp: tm_align(x, y, gen, gen, pp, max_len=max_len)["tm"]
    else:
        score = lambda x, y, pp: tm_score(x, y, gen, gen, pp)["tm"]
    tm = score(final["trans"], final["trans_1"], diag)
    aar = superpose(final["trans"], final["trans_1"], gen, gen, diag, aa_x=final["seqs"], aa_y=final["seqs_1"])["ident"]
    novel = (tm < novelty_tm) & (aar < novelty_ident)

    lab = labels.to(dev)
    glab, gsam = torch.unique(lab, sorted=True, return_inverse=True)
    G = glab.numel()
    novelty = _group_sum(novel, gsam, G) / _group_sum(torch.ones_like(gsam), gsam, G)

    pairs, gidx, _ = group_pairs(labels)
    gidx = gidx.to(dev)
    ptm = score(final["trans"], final["trans"], pairs)
    div_tm = 1.0 - _group_sum(ptm, gidx, G) / _group_sum(torch.ones_like(gidx), gidx, G)
    return {"tm": tm, "tm_pooled": tm.double().mean(), "novel": novel, "novelty": novelty, "diversity_tm": div_tm,
            "group_labels": glab}


def sequence_scores(final, batch, groups=None, known=None, novelty_ident=0.5, **align):
    """The sequence side of the evaluation for peptides of any length: the reference's `diff_ratio` (eval/geometry.py: the
    difflib.SequenceMatcher ratio), an alignment identity and, against a library of known sequences, the nearest known peptide.
    final / batch / groups as in `evaluate_samples` (final["trans"], ["trans_1"], ["seqs"], ["seqs_1"] and batch["generate_mask"] are
    read).  A sample's sequence is its generated residues, in order, at most geometry.SEQ_MAX_LEN = 64 of them (above: NaN).
    **align: mode, matrix, gap_open, gap_extend of geometry.sequence_align (global, +1 / -1, 2, 1).

    -> dict of device tensors:
      seq_ratio       [B] float64: SequenceMatcher(None, sample, native).ratio(), the argument order of diff_ratio(sample, native),
                      bit-equal to difflib's;
      aar             [B] positional identity, as `evaluate_samples` gives it;
      align_identity  [B] float64: identical columns over all columns of the alignment of the sample with the native;
      diversity_seq   [G] float64: 1 - the mean ratio over the pairs i < j of the group (a = sample i, b = sample j), NaN for a group
                      of one;
      group_labels    [G];
    with known = (db_aa [D,Ld], db_len [D]), a library of compact sequences (geometry.sequence_search):
      nearest_known   [B] int32: the entry with the highest alignment score against the sample (lowest index of equal scores; -1 for
                      an empty library);
      nearest_identity [B] float64: the identity of that alignment;
      novel_seq       [B] bool: nearest_identity < novelty_ident (False where there is no nearest entry).
    `diversity_seq`, `novel_seq` and the thresholds are this package's definitions."""
    labels = _check_groups(batch["generate_mask"], groups)
    dev = _device(batch["generate_mask"], final["trans"])
    final = {k: final[k].to(dev) for k in ("trans", "seqs", "trans_1", "seqs_1")}
    B = final["seqs"].shape[0]
    gen = batch["generate_mask"].to(dev).bool()
    ids = torch.arange(B, dtype=torch.int32)
    diag = torch.stack([ids, ids], 1)

    ratio = geometry.sequence_ratio(final["seqs"], final["seqs_1"], gen, gen, diag)["ratio"]
    ident = geometry.sequence_align(final["seqs"], final["seqs_1"], gen, gen, diag, **align)["identity"]
    aar = superpose(final["trans"], final["trans_1"], gen, gen, diag, aa_x=final["seqs"], aa_y=final["seqs_1"])["ident"]

    pairs, gidx, glab = group_pairs(labels)
    gidx = gidx.to(dev)
    G = glab.numel()
    pr = geometry.sequence_ratio(final["seqs"], final["seqs"], gen, gen, pairs)["ratio"]
    div_seq = 1.0 - _group_sum(pr, gidx, G) / _group_sum(torch.ones_like(gidx), gidx, G)
    out = {"seq_ratio": ratio, "aar": aar, "align_identity": ident, "diversity_seq": div_seq, "group_labels": glab.to(dev)}
    if known is not None:
        db_aa, db_len = known
        near = geometry.sequence_search(final["seqs"], gen, db_aa.to(dev), torch.as_tensor(db_len).to(dev), **align)
        out["nearest_known"], out["nearest_identity"] = near["best_index"], near["best_identity"]
        out["novel_seq"] = near["best_identity"] < novelty_ident
    return out


CLUSTER_METRICS = ("rmsd", "pose_rmsd", "tm", "tmalign")
# this package's own default cutoffs, not taken from a publication or a program: 2.0 A for the two RMSDs, 0.5 for the two TM distances
CLUSTER_CUTOFFS = {"rmsd": 2.0, "pose_rmsd": 2.0, "tm": 0.5, "tmalign": 0.5}


def cluster_samples(final, batch, groups=None, metric="rmsd", cutoff=None, method="gromos", score=None):
    """Structural clusters of the samples of each complex, from `sample()` output to cluster labels without leaving the device.
    final / batch / groups as in `evaluate_samples` (only final["trans"] and batch["generate_mask"] are read): the points are the
    sampled CAs over the generated residues.

    metric: the distance between two samples of one group --
      "rmsd"       CA RMSD after the optimal proper superposition (geometry.pairwise_superpose_rmsd);
      "pose_rmsd"  CA RMSD without superposition, in the receptor's frame (superpose's rmsd_plain): what docking pose clustering uses;
      "tm"         1 - TM-score with the correspondence fixed (geometry.pairwise_tm_score);
      "tmalign"    1 - TM-align's score (geometry.pairwise_tm_align).
    cutoff: None takes CLUSTER_CUTOFFS[metric] -- 2.0 A for the two RMSDs, 0.5 for the two TM distances; these defaults are this
    package's own choices.  method: one of geometry.CLUSTER_METHODS; "gromos" follows Daura et al. 1999 and is not checked against
    GROMACS, the linkages are checked against scipy's fcluster(criterion="distance") as partitions only.
    score [B] (optional, lower is better; `binding_energy`'s total or a relaxed energy): adds `best`.

    -> the dict of `geometry.cluster` (label, cluster_size, representative, best, n_neighbours, n_clusters, index, offsets,
    group_labels, group_of) and dist [B,B] (NaN across groups), cluster_diversity [G] float64 = n_clusters / the group's size."""
    if metric not in CLUSTER_METRICS:
        raise ValueError(f"metric must be one of {CLUSTER_METRICS}, got {metric!r}")
    labels = _check_groups(batch["generate_mask"], groups)
    dev = _device(batch["generate_mask"], final["trans"])
    x = final["trans"].to(dev)
    gen = batch["generate_mask"].to(dev).bool()
    B = x.shape[0]
    if metric == "rmsd":
        dist = geometry.pairwise_superpose_rmsd(x, gen, groups=labels)
    elif metric == "pose_rmsd":
        pairs = geometry._within_groups(B, labels)
        dist = geometry._mirrored(B, pairs, dev, (superpose(x, x, gen, gen, pairs)["rmsd_plain"], 0.0))[0]
    elif metric == "tm":
        dist = 1.0 - geometry.pairwise_tm_score(x, gen, groups=labels)
    else:
        dist = 1.0 - geometry.pairwise_tm_align(x, gen, groups=labels)
    out = geometry.cluster(dist, CLUSTER_CUTOFFS[metric] if cutoff is None else cutoff, groups=labels, method=method, score=score)
    out["dist"] = dist
    out["cluster_diversity"] = out["n_clusters"].double() / (out["offsets"][1:] - out["offsets"][:-1]).double()
    return out


def secondary_structure(final, batch, backbone="full_atom"):
    """DSSP of the peptide chain of each sample and of its native, and the secondary-structure ratio of eval/geometry.py:79-91
    (`get_second_stru` / `get_ss`: mdtraj's simplified codes, the fraction of peptide residues that agree).  final / batch as in
    `evaluate_samples`; the peptide chain is generate_mask & res_mask.

    backbone: "full_atom" -- the sample's N, CA, C, O from full_atom_reconstruction(rotmats, trans, angles, seqs), as save_samples_sc
    writes them; "frames" -- from reconstruct_backbone(rotmats, trans, seqs, chain_nb, res_nb, res_mask), as save_samples_bb does;
    "packed" -- the same backbone as "frames" (packing places side chains and leaves N, CA, C, O where they are).
    Prolines come from seqs for the sample and from seqs_1 for the native, whose backbone is pos_heavyatom[..., :4, :]; a native
    residue missing one of those four atoms in mask_heavyatom counts as masked (and never agrees).

    -> dict of device tensors: ss_sample, ss_native [B,L] uint8 8-state codes (255 off the peptide); ssr [B] the fraction of
    generated residues whose simplified codes agree (NaN for a sample without any); ssr_pooled the mean of ssr over the samples
    that have generated residues (float64 scalar); helix, strand, coil [B] the fractions of the sample's generated residues with
    simplified code H, E, C."""
    _check_backbone(backbone)
    dev = _device(batch["generate_mask"], final["trans"], batch["pos_heavyatom"])
    gen = batch["generate_mask"].to(dev).bool() & batch["res_mask"].to(dev).bool()
    chain = batch["chain_nb"].to(dev) if "chain_nb" in batch else None
    rotmats, trans, seqs = (final[k].to(dev) for k in ("rotmats", "trans", "seqs"))
    if backbone == "full_atom":
        bb = full_atom.full_atom_reconstruction(rotmats, trans, final["angles"].to(dev), seqs)[0]
    else:
        bb = full_atom.reconstruct_backbone(rotmats, trans, seqs, batch["chain_nb"].to(dev), batch["res_nb"].to(dev),
                                            batch["res_mask"].to(dev))
    pos = batch["pos_heavyatom"].to(dev)
    native_ok = gen & batch["mask_heavyatom"].to(dev)[:, :, :4].bool().all(-1)
    ss_s = dssp(bb, gen, chain, seqs)
    ss_n = dssp(pos, native_ok, chain, final["seqs_1"].to(dev))
    s_s, s_n = ss_simplify(ss_s), ss_simplify(ss_n)
    n = gen.sum(1).double()
    ssr = ((s_s == s_n) & native_ok).sum(1).double() / n
    frac = [((s_s == c) & gen).sum(1).double() / n for c in range(3)]
    pooled = torch.nan_to_num(ssr).sum() / (n > 0).sum()
    return {"ss_sample": ss_s, "ss_native": ss_n, "ssr": ssr, "ssr_pooled": pooled,
            "helix": frac[0], "strand": frac[1], "coil": frac[2]}


def residue_index(chain_nb, res_nb, res_mask):
    """-> [B,L] int32: 0 at the first residue, + 1 for a step to the next residue of the same chain (both in res_mask, res_nb
    growing by 1), + 2 for any other step.  Indices are unique and increasing, and grow by exactly 1 between bonded neighbours only."""
    ok = res_mask.bool()
    bonded = (chain_nb[:, 1:] == chain_nb[:, :-1]) & (res_nb[:, 1:] - res_nb[:, :-1] == 1) & ok[:, 1:] & ok[:, :-1]
    step = torch.where(bonded, 1, 2).to(torch.int32)
    return torch.cat([torch.zeros_like(step[:, :1]), torch.cumsum(step, 1, dtype=torch.int32)], 1)


def structural_violations(final, batch, backbone="full_atom", scope="generated"):
    """Clashes and broken peptide bonds of each sample's complex and of its native: AlphaFold's between-residue structural
    violations (geometry.structural_violations; the within-residue part is left out).  final / batch as in `evaluate_samples`
    (batch also chain_nb, res_nb).

    backbone: "full_atom" -- generated residues rebuilt with all heavy atoms (reconstruct_sample: rotmats, trans, angles, seqs), the
    context kept; "frames" -- generated residues rebuilt as N, CA, C, O (reconstruct_sample_bb).  The native complex is pos_heavyatom /
    mask_heavyatom / seqs_1.  residue_index comes from `residue_index`, group = generate_mask.
    scope: "generated" -- only atom pairs with an atom in a generated residue are evaluated (query = generate_mask); "all" -- every
    pair, so context residues clashing with each other show in the per-atom arrays too.

    -> dict of device tensors.  Per sample [B], fractions of the generated residues (NaN for a sample without any):
      bond_violation   a peptide bond or bond angle to a neighbour off by more than 12 standard deviations;
      ca_ca_break      CA more than 3.80 + 1.5 A from the next residue's CA;
      clash            an atom overlapping an atom of another residue by more than 1.5 A;
      clash_receptor   such an overlap with an atom of a context residue;  clash_internal  with one of another generated residue;
      violation        any of bond_violation / clash (the reference's violations_per_residue without the within-residue term);
    valid [B] bool: no generated residue has a violation or a CA-CA break; valid_fraction: the mean of valid over the samples that
    have generated residues (float64 scalar); n_clashing_atoms [B] clashing atoms of generated residues.  The same keys with
    `_native` appended for the native complex.  Arrays of the sample (and `*_native`): residue_bond_violation, residue_ca_ca_break,
    residue_clash [B,L] bool, atom_clash, atom_clash_receptor [B,L,14] bool, atom_clash_loss [B,L,14]; residue_index [B,L]."""
    if scope not in ("generated", "all"):
        raise ValueError(f"scope must be 'generated' or 'all', got {scope!r}")
    _, res_mask, gen, index, sample, native = _complexes(final, batch, backbone, index=True)
    query = gen if scope == "generated" else None
    n = gen.sum(1).double()
    has = n > 0
    out = {"residue_index": index}
    for tag, (pos, mask, aa) in (("", sample), ("_native", native)):
        v = geometry.structural_violations(pos, mask & res_mask[:, :, None], aa, index, query=query, group=gen)
        bond, brk = v["connection_violation"], v["ca_ca_break"]
        brk = brk | torch.nn.functional.pad(brk[:, :-1], (1, 0))           # a break counts for both of its residues
        clash, cross = v["clash_atom"].any(-1), v["clash_atom_cross"].any(-1)
        # the generated residues on their own: every partner is generated
        inner = geometry.structural_violations(pos, mask & gen[:, :, None], aa, index)["clash_atom"].any(-1)
        frac = lambda m: torch.where(has, (m & gen).sum(1).double() / n, torch.full_like(n, float("nan")))  # noqa: E731
        any_v = bond | clash
        valid = ~((any_v | brk) & gen).any(1)
        res = {"bond_violation": frac(bond), "ca_ca_break": frac(brk), "clash": frac(clash), "clash_receptor": frac(cross),
               "clash_internal": frac(inner), "violation": frac(any_v), "valid": valid,
               "valid_fraction": (valid & has).sum().double() / has.sum(),
               "n_clashing_atoms": (v["clash_atom"] & gen[:, :, None]).sum((1, 2)),
               "residue_bond_violation": bond, "residue_ca_ca_break": brk, "residue_clash": clash, "atom_clash": v["clash_atom"],
               "atom_clash_receptor": v["clash_atom_cross"], "atom_clash_loss": v["clash_atom_loss"]}
        out.update({k + tag: t for k, t in res.items()})
    return out


def apolar_table():
    """-> [21,15] bool CPU tensor: heavy-atom slot s of residue type t is a carbon or a sulfur (the first letter of the slot's atom
    name; row 20, any type outside 0..19: CA and C)."""
    from .preprocess import _tables
    names = _tables()["atom_names"]
    tab = torch.zeros(21, geometry.SASA_SLOTS, dtype=torch.bool)
    for t in range(20):
        for s in range(geometry.SASA_SLOTS):
            tab[t, s] = bool(names[t][s]) and names[t][s][0] in "CS"
    tab[20, 1] = tab[20, 2] = True
    return tab


def interface_area(final, batch, backbone="full_atom", probe_radius=1.4, n_points=960, min_buried=1.0):
    """Solvent-accessible surface of each sample's peptide, free and bound, and the area buried between peptide and receptor
    (geometry.sasa: Shrake-Rupley over the heavy atoms, Bondi radii), for the sample's complex and for its native.  final / batch and
    the two complexes are those of `structural_violations`: backbone "full_atom" -- generated residues rebuilt with all heavy atoms,
    the context kept; "frames" -- generated residues as N, CA, C, O only; the native is pos_heavyatom / mask_heavyatom / seqs_1.
    group = generate_mask & res_mask: the peptide on its own and the receptor on its own against the complex, in one kernel pass.

    -> dict of device tensors.  Per sample [B], float64, in A^2:
      sasa_peptide_free    surface of the generated residues without the receptor;  sasa_peptide_bound  in the complex;
      buried_peptide       free - bound;  buried_receptor  the same for the context residues;  bsa  the sum of the two;
      buried_fraction      buried_peptide / sasa_peptide_free (NaN for a sample without generated residues);
      buried_apolar_fraction  the share of bsa on carbon and sulfur atoms (NaN where bsa is 0);
      n_interface_peptide, n_interface_receptor  residues that bury more than min_buried A^2;
      interface_recovery   |S_sample & S_native| / (|S_native| + 1e-10) over the receptor's interface residues.
    Per residue [B,L]: residue_buried (float64), interface_residue (bool).  Every key also with `_native` appended (the native's
    interface_recovery is that of the native against itself).  Relative accessibility is not computed."""
    geometry.sphere_points(n_points)                # checks n_points
    if not float(probe_radius) >= 0.0 or not float(min_buried) >= 0.0:
        raise ValueError(f"probe_radius and min_buried must be >= 0, got {probe_radius}, {min_buried}")
    dev, res_mask, gen, _, sample, native = _complexes(final, batch, backbone)
    rec = res_mask & ~gen
    apolar_tab = geometry._table("apolar", dev, apolar_table)
    has = gen.any(1)
    nan = torch.full((gen.shape[0],), float("nan"), dtype=torch.float64, device=dev)
    out, site = {}, {}
    for tag, (pos, mask, aa) in (("", sample), ("_native", native)):
        v = geometry.sasa(pos, mask & res_mask[:, :, None], aa, group=gen, probe_radius=probe_radius, n_points=n_points)
        S = v["sasa_atom"].shape[2]
        buried_atom = v["sasa_atom_own"].double() - v["sasa_atom"].double()
        buried = buried_atom.sum(-1)
        apolar = apolar_tab[torch.where((aa < 0) | (aa > 19), 20, aa)][:, :, :S]
        over = lambda x, m: (x * m).sum(1)  # noqa: E731
        free, bound = over(v["sasa_atom_own"].double().sum(-1), gen), over(v["sasa_atom"].double().sum(-1), gen)
        b_pep, b_rec = over(buried, gen), over(buried, rec)
        bsa = b_pep + b_rec
        face = buried > float(min_buried)
        site[tag] = face & rec
        res = {"sasa_peptide_free": free, "sasa_peptide_bound": bound, "buried_peptide": b_pep, "buried_receptor": b_rec, "bsa": bsa,
               "buried_fraction": torch.where(has, b_pep / free, nan),
               "buried_apolar_fraction": (buried_atom * apolar).sum((1, 2)) / bsa,
               "n_interface_peptide": (face & gen).sum(1), "n_interface_receptor": site[tag].sum(1),
               "residue_buried": buried, "interface_residue": face}
        out.update({k + tag: t for k, t in res.items()})
    n_native = site["_native"].sum(1).double()
    out["interface_recovery"] = (site[""] & site["_native"]).sum(1).double() / (n_native + 1e-10)
    out["interface_recovery_native"] = n_native / (n_native + 1e-10)
    return out


CIS_OMEGA_DEG = 30.0        # an omega within 30 degrees of 0 is a cis peptide bond


def sidechain_packing(final, batch, correct_tol_deg=20.0):
    """Side-chain packing of each sample against its native: the chi1-chi4 errors and the share of residues whose chi angles are all
    within correct_tol_deg (geometry.torsion_angles on both structures, geometry.sidechain_compare on the diagonal).  final / batch as
    in `structural_violations`: the sample is reconstruct_sample(rotmats, trans, angles, seqs) with types where(generate, seqs,
    seqs_1), the native pos_heavyatom / mask_heavyatom / seqs_1; bonded neighbours come from `residue_index`.  Only generated residues
    count.  A chi is compared where both structures define it and the residue types are equal, so the table is that of a
    `sample(..., sample_bb=False, sample_seq=False)` run; with sampled sequences it covers the recovered positions.  The pi-periodic
    chi (geometry.PI_PERIODIC_CHI) are compared modulo pi.

    -> dict of device tensors.  Per sample, in degrees, NaN where nothing is compared: chi_mae [B,4], chi_correct [B,4] (the share
    within the tolerance), residue_correct [B] (residues with every compared chi within it, over residues with a compared chi),
    psi_o_mae, phi_mae, psi_mae [B] (psi_o: the N-CA-C-O angle, which is the model's first angle + pi), sc_rmsd [B] (side-chain atoms
    in the backbone frame, equivalent atoms exchanged where that is closer, in A), n_chi [B,4] int32, cis_fraction [B] (the sample's
    defined omegas of generated residues within 30 degrees of 0).  Pooled over the compared residues of the batch, float64:
    chi_mae_pooled [4], chi_correct_pooled [4], residue_correct_pooled.  By the native's residue type: chi_mae_by_type [20,4]
    (float64), n_chi_by_type [20,4].  Per residue: chi_err [B,L,4] (degrees, NaN where not compared), residue_sc_rmsd [B,L] (NaN
    where no atom is compared), swapped [B,L] bool, angles_sample, angles_native [B,L,8] (radians, geometry.TORSION_NAMES; before
    the restriction to generated residues)."""
    tol = float(correct_tol_deg)
    if not 0.0 <= tol <= 180.0:
        raise ValueError(f"correct_tol_deg must be in [0, 180], got {correct_tol_deg}")
    dev, res_mask, gen, index, sample, native = _complexes(final, batch, "full_atom", index=True)
    seqs_1 = native[2]
    B, L = gen.shape
    sides = []
    for pos, mask, aa in (sample, native):
        t = geometry.torsion_angles(pos, mask & res_mask[:, :, None], aa, index)
        sides.append(dict(pos=pos, atom_mask=mask & gen[:, :, None], aa=aa, angles=t["angles"], defined=t["defined"] & gen[:, :, None]))
    ids = torch.arange(B, dtype=torch.int32, device=dev)
    c = geometry.sidechain_compare(sides[0], sides[1], torch.stack([ids, ids], 1), correct_tol=math.radians(tol), per_residue=True)

    deg = 180.0 / math.pi
    cnt = c["err_count"].double()
    mae = c["err_sum"] * deg / cnt                          # 0 / 0: NaN where nothing is compared
    share = c["within"].double() / cnt
    omega, om_def = sides[0]["angles"][:, :, 0], sides[0]["defined"][:, :, 0]
    cis = om_def & ((omega <= math.radians(CIS_OMEGA_DEG)) | (omega >= math.radians(360.0 - CIS_OMEGA_DEG)))
    chi_err = c["err"][:, :, 4:] * deg
    compared = ~torch.isnan(chi_err)
    types = seqs_1.clamp(0, 19).reshape(-1)
    by_sum = _group_sum(torch.nan_to_num(chi_err).reshape(-1, 4), types, 20)
    by_n = _group_sum(compared.reshape(-1, 4), types, 20, dtype=torch.int64)
    sc_n = c["sc_n"].double()
    return {"chi_mae": mae[:, 4:], "chi_correct": share[:, 4:], "residue_correct": c["res_correct"].double() / c["res_with_chi"].double(),
            "psi_o_mae": mae[:, 3], "phi_mae": mae[:, 1], "psi_mae": mae[:, 2], "sc_rmsd": c["sc_rmsd"], "n_chi": c["err_count"][:, 4:],
            "cis_fraction": cis.sum(1).double() / om_def.sum(1).double(),
            "chi_mae_pooled": c["err_sum"][:, 4:].sum(0) * deg / cnt[:, 4:].sum(0),
            "chi_correct_pooled": c["within"][:, 4:].sum(0).double() / cnt[:, 4:].sum(0),
            "residue_correct_pooled": c["res_correct"].sum().double() / c["res_with_chi"].sum().double(),
            "chi_mae_by_type": by_sum / by_n.double(), "n_chi_by_type": by_n,
            "chi_err": chi_err, "residue_sc_rmsd": torch.sqrt(c["sc_sq"].double() / sc_n).float(), "swapped": c["swapped"],
            "angles_sample": sides[0]["angles"], "angles_native": sides[1]["angles"]}


def _mean_of_defined(v):
    """the mean of v [B] over its entries that are not NaN (NaN when there is none), float64"""
    has = ~torch.isnan(v)
    return torch.nan_to_num(v.double()).sum() / has.sum().double()


def local_accuracy(final, batch, backbone="full_atom", cutoff=15.0):
    """lDDT of each sample's generated residues against the native complex: a local accuracy that needs no superposition
    (geometry.lddt, the values of OpenFold's lddt / lddt_ca).  final / batch and the two complexes are those of `structural_violations`:
    backbone "full_atom" -- generated residues rebuilt with all heavy atoms, the context kept; "frames" -- generated residues as N, CA,
    C, O only (lddt_all then covers those atoms).  Rows are the generated residues (query = generate_mask & res_mask), every residue of
    the complex is a partner, group = the same mask.  Atom pairs inside a residue are scored, as the reference scores them.

    -> dict of device tensors.  Per sample [B], float64, NaN for a sample without generated residues (or without a scored pair):
      lddt_ca, lddt_backbone, lddt_all     over CA; N, CA, C, O; all heavy atoms (side chains where the residue types agree);
      ilddt_ca, ilddt_backbone, ilddt_all  the same over the pairs across the groups only: does the peptide keep its distances to
                                           the receptor (this package's name for it);
    per residue: lddt_residue [B,L] (all atoms, NaN off the generated residues); pooled: lddt_ca_pooled, lddt_backbone_pooled,
    lddt_all_pooled and the three ilddt_*_pooled, the mean over the samples that have a value (float64 scalars)."""
    cutoff = float(cutoff)
    dev, res_mask, gen, _, sample, native = _complexes(final, batch, backbone)
    x, y = (dict(pos=pos, atom_mask=mask & res_mask[:, :, None], aa=aa) for pos, mask, aa in (sample, native))
    ids = torch.arange(gen.shape[0], dtype=torch.int32, device=dev)
    diag = torch.stack([ids, ids], 1)
    out = {}
    for name in ("ca", "backbone", "all"):
        v = geometry.lddt(x, y, diag, slots=name, cutoff=cutoff, group=gen, query=gen)
        out["lddt_" + name], out["ilddt_" + name] = v["lddt"], v["lddt_cross"]
        out["lddt_" + name + "_pooled"], out["ilddt_" + name + "_pooled"] = _mean_of_defined(v["lddt"]), _mean_of_defined(v["lddt_cross"])
    out["lddt_residue"] = v["lddt_residue"]
    return out


def docking_quality(final, batch, backbone="full_atom", contact_cutoff=5.0, interface_cutoff=10.0):
    """DockQ of each sample's peptide on its receptor against the native complex (geometry.dockq: Basu & Wallner 2016, written from
    the publication and not checked against the DockQ program).  final / batch and the two complexes are those of
    `structural_violations`; the ligand is generate_mask & res_mask, the receptor the other residues of res_mask.  With
    backbone="frames" the sample's generated residues have N, CA, C, O only while the native keeps its side chains, so the sample's
    contacts -- and with them fnat -- are undercounted; "full_atom" is the default.  The CAPRI-peptide cut-offs are
    contact_cutoff=4.0, interface_cutoff=8.0.

    -> dict of device tensors.  Per sample [B]: fnat, fnonnat, irmsd, lrmsd, dockq (float64; NaN for a sample without native
    contacts), dockq_class (int64, 0 incorrect .. 3 high), n_native_contacts, n_sample_contacts (int64, residue pairs).  Pooled, this
    package's pooling: dockq_pooled, the mean over the samples that have a value, and success_rate, the share of those with DockQ >=
    0.23 (float64 scalars)."""
    dev, res_mask, gen, _, sample, native = _complexes(final, batch, backbone)
    x, y = (dict(pos=pos, atom_mask=mask & res_mask[:, :, None], aa=aa) for pos, mask, aa in (sample, native))
    ids = torch.arange(gen.shape[0], dtype=torch.int32, device=dev)
    d = geometry.dockq(x, y, torch.stack([ids, ids], 1), gen, contact_cutoff=contact_cutoff, interface_cutoff=interface_cutoff)
    out = {k: d[k] for k in ("fnat", "fnonnat", "irmsd", "lrmsd", "dockq", "dockq_class", "n_native_contacts", "n_sample_contacts")}
    has = ~torch.isnan(d["dockq"])
    out["dockq_pooled"] = _mean_of_defined(d["dockq"])
    out["success_rate"] = (has & (d["dockq"] >= 0.23)).sum().double() / has.sum().double()
    return out


ROT_PER_RESIDUE = 2         # phi and psi: the backbone's share of a generated residue in n_rot
ROT_PENALTY = 0.0585        # Trott & Olson's weight of the rotatable-bond count


def binding_energy(final, batch, backbone="full_atom", cutoff=8.0):
    """An empirical affinity proxy for each sample: geometry.interface_energy -- the functional form of AutoDock Vina's scoring
    function (Trott & Olson, J. Comput. Chem. 2010) over heavy atoms, with geometry.VINA_WEIGHTS -- between the peptide and its
    receptor, for the sample's complex and for its native.  It is written from the publication and checked against a float64
    restatement in this tree; it is not checked against the Vina program, and it stands in for, but is not, the Rosetta dG_separated
    or FoldX value of the reference's evaluation.  final / batch and the two complexes are those of `structural_violations`; the
    peptide is generate_mask & res_mask, the receptor the other residues of res_mask; padding residues have no atoms.  With
    backbone="frames" the sample's generated residues have N, CA, C, O only: a backbone-only score, which the native (with its side
    chains) is then not comparable with.

    -> dict of device tensors.  Per sample [B], float64: energy, energy_native, delta = energy - energy_native; terms, terms_native
    [B,5] (unweighted, geometry.ENERGY_TERMS); energy_per_rot = energy / (1 + 0.0585 n_rot).  n_hbonds, n_hydrophobic [B] int64: the
    sample's atom pairs with hbond > 0 / hydrophobic > 0, summed over the peptide's rows.  n_rot [B] int64 = the sum over the
    generated residues of (the number of chi angles of the sample's type, from the package's chi table, + 2 for phi and psi): this
    package's convention for a peptide's rotatable bonds, not Vina's torsion tree.  clashing [B] bool: w_repulsion * repulsion >
    |w_gauss1 * gauss1 + w_gauss2 * gauss2| on the sample's terms, i.e. the steric penalty outweighs the steric attraction.  Per
    residue [B,L] float32: energy_residue, energy_residue_native (the rows of the peptide and of the receptor, each pair in both of
    its rows; 0 elsewhere)."""
    dev, res_mask, gen, _, sample, native = _complexes(final, batch, backbone)
    out = {}
    for tag, (pos, mask, aa) in (("", sample), ("_native", native)):
        v = geometry.interface_energy(pos, mask & res_mask[:, :, None], aa, gen, cutoff=cutoff)
        out["energy" + tag], out["terms" + tag], out["energy_residue" + tag] = v["energy"], v["terms"], v["energy_residue"]
        if not tag:
            over = lambda t: (t.to(torch.int64).sum(-1) * gen).sum(1)  # noqa: E731
            out["n_hbonds"], out["n_hydrophobic"] = over(v["hbond_pairs_atom"]), over(v["hydrophobic_pairs_atom"])
    out["delta"] = out["energy"] - out["energy_native"]
    aa_s = sample[2]
    n_chi = (geometry._table("chi_atoms", dev, geometry.chi_atom_table)[:, :, 0] >= 0).sum(1)          # [21]
    out["n_rot"] = ((n_chi[torch.where((aa_s < 0) | (aa_s > 20), 20, aa_s)] + ROT_PER_RESIDUE) * gen).sum(1)
    out["energy_per_rot"] = out["energy"] / (1.0 + ROT_PENALTY * out["n_rot"].double())
    w, t = geometry.VINA_WEIGHTS, out["terms"]
    out["clashing"] = w[2] * t[:, 2] > (w[0] * t[:, 0] + w[1] * t[:, 1]).abs()
    return out


def _bonded_residue_pairs(partner, gen):
    """hbond_partner [B,L,15,K] -> [B,L,L] bool: residues i, j of different sides (gen) joined by a listed hydrogen bond.  A bond is
    in the list of both of its atoms, so one that an atom's list of the 4 lowest partners drops is still seen from the other row."""
    B, L = gen.shape
    res = torch.div(partner.clamp(min=0), geometry.POLAR_SLOTS, rounding_mode="floor").long().reshape(B, L, -1)
    hits = torch.zeros(B, L, L, dtype=torch.int32, device=gen.device)
    hits.scatter_add_(2, res, (partner >= 0).reshape(B, L, -1).to(torch.int32))        # integer sums: the same from run to run
    pairs = hits > 0
    pairs = pairs | pairs.transpose(1, 2)
    return pairs & (gen[:, :, None] != gen[:, None, :])


def polar_satisfaction(final, batch, backbone="full_atom", max_sasa=1.0, probe_radius=1.4, n_points=960, **criteria):
    """Polar chemistry at the interface of each sample's complex and of its native: directional hydrogen bonds and salt bridges
    between peptide and receptor (geometry.polar_interactions) and the polar atoms buried at the interface without a hydrogen-bond
    partner (joined with geometry.sasa), the filter that the reference's evaluation takes from Rosetta's interface analysis
    (hbonds_int, delta_unsatHbonds).  Heavy atoms only, by the published heavy-atom conventions (Baker & Hubbard 1984, McDonald &
    Thornton 1994, Barlow & Thornton 1983), written from the publications and checked against a float64 restatement in this tree; it
    is not checked against HBPLUS, PLIP or Rosetta and is not Rosetta's count.  final / batch and the two complexes are those of
    `structural_violations`; group = generate_mask & res_mask; one polar_interactions call and one sasa call per complex; `criteria`
    (d_max, acc_angle_min, don_angle_min, salt_max, his_charged) go to polar_interactions.  With backbone="frames" the sample's
    generated residues have N, CA, C, O only: it then reports the backbone's polar atoms only, which the native (with its side
    chains) is not comparable with.

    A polar atom is a participating donor or acceptor (geometry.interface_type_table).  It is buried when its accessible area in the
    complex is <= max_sasa, and unsatisfied when it has no hydrogen bond at all (hbonds_atom == 0).  max_sasa = 1.0 A^2 is a starting
    value, not a tuned one.  The interface holds the peptide and the receptor residues that bury more than 1 A^2, as in
    `interface_area`.

    -> dict of device tensors.  Per sample [B], int64:
      n_hbonds_interface, n_salt_bridges_interface   hydrogen bonds / salt-bridge atom pairs between peptide and receptor;
      n_hbonds_peptide       hydrogen bonds with both atoms in the peptide;
      n_buried_unsat         buried unsatisfied polar atoms of the interface;
      n_buried_unsat_delta   those of them that are exposed (area > max_sasa) in their own side alone: buried by binding;
    hbond_recovery [B] float64: |P_sample & P_native| / (|P_native| + 1e-10) over the residue pairs P joined by a hydrogen bond
    across the interface.  Per residue [B,L] int32: buried_unsat.  Every key also with `_native` appended (the native's
    hbond_recovery is that of the native against itself)."""
    max_sasa = float(max_sasa)
    if not max_sasa >= 0.0:
        raise ValueError(f"max_sasa must be >= 0, got {max_sasa}")
    dev, res_mask, gen, index, sample, native = _complexes(final, batch, backbone, index=True)
    rec = res_mask & ~gen
    types = geometry._table("interface_types", dev, geometry.interface_type_table)
    S = geometry.POLAR_SLOTS
    out, bonded = {}, {}
    for tag, (pos, mask, aa) in (("", sample), ("_native", native)):
        mask = mask & res_mask[:, :, None]
        p = geometry.polar_interactions(pos, mask, aa, index, group=gen, **criteria)
        v = geometry.sasa(pos, mask, aa, group=gen, probe_radius=probe_radius, n_points=n_points)
        bits = types[torch.where((aa < 0) | (aa > 19), 20, aa)]
        part = torch.zeros_like(bits, dtype=torch.bool)
        part[:, :, :mask.shape[2]] = mask[:, :, :S]
        polar = ((bits & (geometry.TYPE_DONOR | geometry.TYPE_ACCEPTOR)) != 0) & part
        face = (v["sasa_atom_own"].double() - v["sasa_atom"].double()).sum(-1) > 1.0
        scope = gen | (face & rec)
        unsat = polar & (v["sasa_atom"] <= max_sasa) & (p["hbonds_atom"] == 0) & scope[:, :, None]
        delta = unsat & (v["sasa_atom_own"] > max_sasa)
        inner = ((p["hbonds_atom"] - p["hbonds_atom_cross"]).sum(-1, dtype=torch.int64) * gen).sum(1) // 2
        bonded[tag] = _bonded_residue_pairs(p["hbond_partner"], gen)
        res = {"n_hbonds_interface": p["n_hbonds_cross"], "n_salt_bridges_interface": p["n_salt_bridges_cross"],
               "n_hbonds_peptide": inner, "n_buried_unsat": unsat.sum((1, 2)), "n_buried_unsat_delta": delta.sum((1, 2)),
               "buried_unsat": unsat.sum(-1, dtype=torch.int32)}
        out.update({k + tag: t for k, t in res.items()})
    n_native = bonded["_native"].sum((1, 2)).double() / 2
    out["hbond_recovery"] = (bonded[""] & bonded["_native"]).sum((1, 2)).double() / 2 / (n_native + 1e-10)
    out["hbond_recovery_native"] = n_native / (n_native + 1e-10)
    return out


def relax_samples(final, batch, backbone="full_atom", steps=200, **params):
    """Restrained relaxation of each sample's complex on the device (geometry.relax: a restraint force field from the clash overlap
    and peptide-bond ideals of `structural_violations` plus the sample's own internal distances, and a monotone minimiser; NOT Amber
    and NOT Rosetta's FastRelax, whose place before the energy it takes in role only), with the clash counts and the interface
    energy before and after.  final / batch and the sample's complex are those of `binding_energy`; the generated residues move, the
    receptor is fixed; steps and params go to geometry.relax.

    -> dict of device tensors: pos_heavyatom [B,L,15,3] float32 (the receptor's atoms bit-identical to the rebuilt complex, i.e. to
    batch["pos_heavyatom"]), mask_heavyatom [B,L,15] bool, rmsd_heavy [B] float64 (the generated residues' atoms against the
    unrelaxed sample); terms_before, terms_after [B,4] float64 (geometry.RELAX_TERMS), relax_energy_before, relax_energy_after,
    energy_trace [B,steps+1], accepted [B,steps], iterations [B]; clash_atoms_before, clash_atoms_after, clash_atoms_cross_before,
    clash_atoms_cross_after [B] int64: the generated residues' atoms that geometry.structural_violations flags, against any other
    residue and against the receptor; energy, energy_relaxed [B] float64 and clashing, clashing_relaxed [B] bool: geometry.
    interface_energy between peptide and receptor and `binding_energy`'s clashing flag, on the sample and on the relaxed complex."""
    _check_backbone(backbone)
    geometry._relax_params(params, steps)                   # checked before final / batch are touched
    dev, res_mask, gen, index, (pos, mask, aa), _ = _complexes(final, batch, backbone, index=True)
    mask = mask & res_mask[:, :, None]
    r = geometry.relax(pos, mask, aa, index, gen, steps=steps, **params)
    out = {"pos_heavyatom": r["pos"], "mask_heavyatom": mask, "rmsd_heavy": r["rmsd"], "terms_before": r["terms_initial"],
           "terms_after": r["terms_final"], "relax_energy_before": r["energy_trace"][:, 0], "relax_energy_after": r["energy_trace"][:, -1],
           "energy_trace": r["energy_trace"], "accepted": r["accepted"], "iterations": r["iterations"]}
    w = geometry.VINA_WEIGHTS
    for tag, etag, p in (("_before", "", pos), ("_after", "_relaxed", r["pos"])):
        v = geometry.structural_violations(p, mask, aa, index, query=gen, group=gen)
        out["clash_atoms" + tag] = (v["clash_atom"] & gen[:, :, None]).sum((1, 2))
        out["clash_atoms_cross" + tag] = (v["clash_atom_cross"] & gen[:, :, None]).sum((1, 2))
        e = geometry.interface_energy(p, mask, aa, gen)
        t = e["terms"]
        out["energy" + etag] = e["energy"]
        out["clashing" + etag] = w[2] * t[:, 2] > (w[0] * t[:, 0] + w[1] * t[:, 1]).abs()
    return out


def pack_samples(final, batch, backbone="frames", **kw):
    """Rotamer side-chain packing of each sample's generated residues against the fixed receptor on the device (geometry.
    pack_sidechains: a staggered rotamer grid unless `rotamers` is given, the pair function of geometry.interface_energy, iterated
    conditional modes; NOT SCWRL4 and NOT Rosetta's packer, whose place before the energies (eval/run_scwrl4.py) it takes in role
    only), with the clash counts and the interface energy before and after and the packing table against the native.  final / batch
    and the sample's complex are those of `binding_energy` with backbone "frames" (the default: a backbone-only run) or "full_atom"
    (the model's own side chains are replaced); movable = generate_mask & res_mask, the index comes from `residue_index`, the types
    are where(generate, seqs, seqs_1); kw (rotamers, sweeps, cutoff, weights) goes to geometry.pack_sidechains.

    -> dict of device tensors: pos_heavyatom [B,L,15,3] float32 (the receptor's atoms bit-identical to the rebuilt complex),
    mask_heavyatom [B,L,15] bool, chi [B,L,4] float32 (radians, the chosen rotamer's), rotamer [B,L] int32 (-1 where not packed),
    energy_trace [B,sweeps+1] float64, sweeps_run [B]; clash_atoms_before, clash_atoms_after, clash_atoms_cross_before,
    clash_atoms_cross_after [B] int64 (the generated residues' atoms that geometry.structural_violations flags, against any other
    residue and against the receptor) and energy_before, energy_after [B] float64 (geometry.interface_energy between peptide and
    receptor), on the complex as given and as packed; chi_mae, chi_correct [B,4] and residue_correct [B] of the packed complex
    against the native (geometry.sidechain_compare, as `sidechain_packing` reports them: degrees, NaN where nothing is compared) --
    the packing baseline to put next to the model's own angles."""
    if backbone not in ("full_atom", "frames"):
        raise ValueError(f"backbone must be 'full_atom' or 'frames', got {backbone!r}")
    if "trace" in kw:
        raise ValueError("pack_samples does not return the choice trace; call geometry.pack_sidechains for it")
    sweeps = kw.get("sweeps", 8)
    if not isinstance(sweeps, int) or isinstance(sweeps, bool) or sweeps < 0:      # checked before final / batch are touched
        raise ValueError(f"sweeps must be an integer >= 0, got {sweeps!r}")
    dev, res_mask, gen, index, (pos, mask, aa), (pos_n, mask_n, aa_n) = _complexes(final, batch, backbone, index=True)
    mask = mask & res_mask[:, :, None]
    r = geometry.pack_sidechains(pos, mask, aa, index, gen, **kw)
    new_mask = torch.where(r["packed"][:, :, None], r["atom_mask"], mask)
    out = {"pos_heavyatom": r["pos"], "mask_heavyatom": new_mask, "chi": r["chi"], "rotamer": r["rotamer"],
           "energy_trace": r["energy_trace"], "sweeps_run": r["sweeps_run"]}
    for tag, p, m in (("_before", pos, mask), ("_after", r["pos"], new_mask)):
        v = geometry.structural_violations(p, m, aa, index, query=gen, group=gen)
        out["clash_atoms" + tag] = (v["clash_atom"] & gen[:, :, None]).sum((1, 2))
        out["clash_atoms_cross" + tag] = (v["clash_atom_cross"] & gen[:, :, None]).sum((1, 2))
        out["energy" + tag] = geometry.interface_energy(p, m, aa, gen)["energy"]
    sides = []
    for p, m, t in ((r["pos"], new_mask, aa), (pos_n, mask_n, aa_n)):
        ang = geometry.torsion_angles(p, m & res_mask[:, :, None], t, index)
        sides.append(dict(pos=p, atom_mask=m & gen[:, :, None], aa=t, angles=ang["angles"], defined=ang["defined"] & gen[:, :, None]))
    ids = torch.arange(gen.shape[0], dtype=torch.int32, device=dev)
    c = geometry.sidechain_compare(sides[0], sides[1], torch.stack([ids, ids], 1))
    deg, cnt = 180.0 / math.pi, c["err_count"].double()
    out["chi_mae"] = (c["err_sum"] * deg / cnt)[:, 4:]
    out["chi_correct"] = (c["within"].double() / cnt)[:, 4:]
    out["residue_correct"] = c["res_correct"].double() / c["res_with_chi"].double()
    return out


HOT_SPOT_DDE = 1.0          # ddE_ala at or above which a residue is called a hot spot: a starting value in this energy's units, not tuned


def _scan_candidate_mask(candidates):
    """"all" | "ALA" | a sequence of three-letter residue names -> None (every type) or a [20] bool mask (ValueError)"""
    from .preprocess import residue_type
    if isinstance(candidates, str):
        if candidates == "all":
            return None
        candidates = (candidates,)
    try:
        names = list(candidates)
    except TypeError:
        raise ValueError(f"candidates must be 'all', 'ALA' or a sequence of residue names, got {candidates!r}") from None
    mask = torch.zeros(geometry.SCAN_TYPES, dtype=torch.bool)
    for n in names:
        t = residue_type(n) if isinstance(n, str) else None
        if t is None or not 0 <= t < geometry.SCAN_TYPES:
            raise ValueError(f"candidates: {n!r} is not one of the 20 residue types")
        mask[t] = True
    if not names:
        raise ValueError("candidates names no residue type")
    return mask


def mutation_scan(final, batch, backbone="packed", candidates="all", hot_spot=HOT_SPOT_DDE, top_k=5, **kw):
    """Point-mutation scanning of each sample's generated residues against the complex as it stands, on the device (geometry.
    mutation_scan: at every generated residue and for every candidate type, the best rotamer's self energy of `pack_sidechains` with
    nothing else moved or repacked, minus the wild type's on the same rotamer grid).  It answers which residues carry the binding (an
    alanine scan: ddE_ala) and which single substitutions would score better (a position scan: ddE, top_*), where the reference's
    evaluation calls FoldX's AlaScan / PositionScan (eval/foldx.py) or Rosetta.  It is NOT FoldX and NOT Rosetta and takes their
    place in role only: this package's Vina-form pair energy, no solvation, no electrostatics, no entropy, no backbone movement;
    ALA and GLY both score 0 and differences in the backbone (PRO's N, GLY's missing CB) do not show; the defaults are untuned.
    final / batch and the sample's complex are those of `binding_energy` (`_complexes`; the default backbone "packed" places the
    side chains first, "frames" scans a backbone-only peptide); positions = generate_mask & res_mask, group = the same mask (so
    *_interface is the part against the receptor), the index comes from `residue_index`, the types are where(generate, seqs, seqs_1).
    candidates: "all", "ALA" or a sequence of three-letter names (the wild type is evaluated besides); hot_spot: the ddE_ala at or
    above which a residue is called a hot spot -- HOT_SPOT_DDE is a starting value, not a tuned one; kw (rotamers, cutoff, weights)
    goes to geometry.mutation_scan.

    -> dict of device tensors: ddE, ddE_interface [B,L,20] float32 (NaN where not evaluated; 0 at the wild type); energy [B,L,20]
    and rotamer [B,L,20] as geometry.mutation_scan gives them; scanned [B,L] bool; ddE_ala [B,L] = ddE[..., ALA]; hot_spot [B,L] bool
    (ddE_ala >= hot_spot); top_position, top_type [B,top_k] int64 and top_ddE [B,top_k] float32: the top_k most favourable
    substitutions of each sample other than the wild type, ascending in ddE (torch.topk; where a sample has fewer candidates the
    rest are position -1, type -1, ddE NaN)."""
    from .preprocess import residue_type
    _check_backbone(backbone)
    cand = _scan_candidate_mask(candidates)
    if not isinstance(top_k, int) or isinstance(top_k, bool) or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k!r}")
    hot_spot = float(hot_spot)
    if math.isnan(hot_spot):
        raise ValueError("hot_spot must be a number")
    dev, res_mask, gen, index, (pos, mask, aa), _ = _complexes(final, batch, backbone, index=True)
    r = geometry.mutation_scan(pos, mask & res_mask[:, :, None], aa, index, gen, candidates=cand, group=gen, **kw)
    B, L, T = r["ddE"].shape
    ala = residue_type("ALA")
    out = {"ddE": r["ddE"], "ddE_interface": r["ddE_interface"], "energy": r["energy"], "rotamer": r["rotamer"], "scanned": r["scanned"],
           "ddE_ala": r["ddE"][:, :, ala]}
    out["hot_spot"] = out["ddE_ala"] >= hot_spot
    wild = torch.arange(T, device=dev)[None, None, :] == aa[:, :, None]
    score = torch.where(torch.isnan(r["ddE"]) | wild, torch.full((), float("inf"), device=dev), r["ddE"]).reshape(B, L * T)
    k = min(top_k, L * T)
    v, at = torch.topk(score, k, dim=1, largest=False, sorted=True)
    found = torch.isfinite(v)
    out["top_position"] = torch.where(found, torch.div(at, T, rounding_mode="floor"), torch.full_like(at, -1))
    out["top_type"] = torch.where(found, at % T, torch.full_like(at, -1))
    out["top_ddE"] = torch.where(found, v, torch.full_like(v, float("nan")))
    return out


def design_sequences(final, batch, backbone="frames", candidates="all", **kw):
    """Fixed-backbone sequence design of each sample's generated residues against the fixed receptor on the device (geometry.
    design_sequence: type and rotamer of every generated residue chosen together by iterated conditional modes over `pack_sidechains`'
    energy).  It answers which sequence this package's own energy prefers on a sampled backbone, where the reference's evaluation
    runs ProteinMPNN over the peptide chain of backbone-only samples (eval/run_mpnn.py: process_mpnn_bb, write_seq_to_pdb).  It is
    NOT ProteinMPNN and NOT Rosetta fixbb and takes their place in role only: this package's Vina-form pair energy plus the rotamer
    table's energy plus the caller's `ref_energy`, no solvation, no electrostatics, no entropy, no learned prior; without reference
    energies it favours large side chains; a local search; the defaults are untuned and no reference energies are shipped.
    final / batch and the sample's complex are those of `binding_energy` with backbone "frames" (the default: a backbone-only run) or
    "full_atom"; designed = generate_mask & res_mask, the receptor is the fixed environment, the index comes from `residue_index`,
    the types are where(generate, seqs, seqs_1).  candidates: "all", "ALA" or a sequence of three-letter names (a [20] set for every
    designed residue); kw (ref_energy, rotamers, sweeps, cutoff, weights) goes to geometry.design_sequence.

    -> dict of device tensors: seqs [B,L] int64 (the designed types; others as given); pos_heavyatom [B,L,15,3] float32 (the
    receptor's atoms bit-identical to the rebuilt complex), mask_heavyatom [B,L,15] bool, chi [B,L,4], rotamer [B,L] int32 (-1 where
    not designed), energy_trace [B,sweeps+1] float64, sweeps_run [B], profile [B,L,20] float32, status [B] int32 (1: more than
    geometry.SEQ_DESIGN_MAX_RES generated residues, nothing designed); recovery_native, recovery_model [B] float64: the share of the
    designed residues whose type equals seqs_1, final["seqs"] (NaN where nothing is designed); changed_from_model [B] int64: designed
    residues whose type differs from final["seqs"]; energy_before, energy_after [B] float64 (geometry.interface_energy between
    peptide and receptor) and clash_atoms_cross_before, clash_atoms_cross_after [B] int64 (the generated residues' atoms that
    geometry.structural_violations flags against the receptor), on the complex as given and as designed."""
    if backbone not in ("full_atom", "frames"):
        raise ValueError(f"backbone must be 'full_atom' or 'frames', got {backbone!r}")
    cand = _scan_candidate_mask(candidates)
    if "trace" in kw:
        raise ValueError("design_sequences does not return the choice trace; call geometry.design_sequence for it")
    sweeps = kw.get("sweeps", 8)
    if not isinstance(sweeps, int) or isinstance(sweeps, bool) or sweeps < 0:      # checked before final / batch are touched
        raise ValueError(f"sweeps must be an integer >= 0, got {sweeps!r}")
    geometry._ref_energy(kw.get("ref_energy"))
    dev, res_mask, gen, index, (pos, mask, aa), (pos_n, mask_n, aa_n) = _complexes(final, batch, backbone, index=True)
    mask = mask & res_mask[:, :, None]
    r = geometry.design_sequence(pos, mask, aa, index, gen, candidates=cand, **kw)
    new_mask = torch.where(r["designed"][:, :, None], r["atom_mask"], mask)
    out = {"seqs": r["aa"], "pos_heavyatom": r["pos"], "mask_heavyatom": new_mask, "chi": r["chi"], "rotamer": r["rotamer"],
           "energy_trace": r["energy_trace"], "sweeps_run": r["sweeps_run"], "profile": r["profile"], "status": r["status"]}
    des = r["designed"]
    count = des.sum(1).double()
    model = final["seqs"].to(dev)
    out["recovery_native"] = (des & (r["aa"] == aa_n)).sum(1).double() / count
    out["recovery_model"] = (des & (r["aa"] == model)).sum(1).double() / count
    out["changed_from_model"] = (des & (r["aa"] != model)).sum(1)
    for tag, p, m, t in (("_before", pos, mask, aa), ("_after", r["pos"], new_mask, r["aa"])):
        v = geometry.structural_violations(p, m, t, index, query=gen, group=gen)
        out["clash_atoms_cross" + tag] = (v["clash_atom_cross"] & gen[:, :, None]).sum((1, 2))
        out["energy" + tag] = geometry.interface_energy(p, m, t, gen)["energy"]
    return out
