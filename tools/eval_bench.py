"""Times the evaluation kernels against the same work done with torch ops and torch.linalg.svd on the device.

Cases: the pairwise superposition at 64 samples x 25 CA (2 016 pairs), the same at 16 groups x 64 samples (32 256 pairs), and
batch_align at B = 64, L = 128, A = 15.  TM-score (pf_tm_score_fwd): pairwise at 64 samples x 15 and x 25 CA (2 016 pairs each), 16 groups
x 64 x 25 (32 256 pairs) and 64 sample-vs-native pairs at N = 128, checked against the float64 oracle of tests/tm_oracle.py on the
CPU (a subset of the pairs; its time per pair is reported).  DSSP (pf_dssp_fwd): 4 096 chains x 25 residues (64 complexes x 64
samples), 64 x 128 and 8 x 512 NeRF chains, checked against the float64 oracle of tests/dssp_oracle.py on a subset of the chains (its
CPU time per chain is reported), and metrics.secondary_structure at 64 samples x 25 generated residues.  TM-align (pf_tm_align_fwd):
pairwise at 64 samples x 25 CA (2 016 pairs), the same peptides inside 128-slot complex tensors (as structure_scores passes them),
16 groups x 64 x 25 (32 256 pairs) and 64 sample-vs-native pairs at N = 128 with unequal lengths, checked against the float64 oracle
of tests/tmalign_oracle.py on a subset (its CPU time per pair is reported).  Structural violations (pf_violations_fwd, `--only
violations` runs this leg alone): the heavy atoms of 64 complexes of 144 and of 512 residues, every pair and with query = the 12
generated residues, against a dense torch restatement of the clash pass ([B,L,L,14,14] tensors) on the device at 8 x 144, and
metrics.structural_violations at 64 x 144.  Solvent-accessible surface (pf_sasa_fwd, `--only sasa`): the same complexes of 144 and of
512 residues at 960 and at 92 points, with and without `group`, metrics.interface_area at 64 x 144, a chunked torch restatement
([atoms, points, partners] tensors, 8 atoms at a time) on the device at 8 x 144, and the CPU time of the float64 oracle of
tests/sasa_oracle.py on one complex.  Torsion angles and side-chain packing (pf_torsions_fwd, pf_sidechain_compare_fwd, `--only
torsions`): 64 complexes of 144 residues, torsion_angles of both structures and sidechain_compare on the diagonal, against
preprocess.get_torsion_angle (the torch-op form: N-CA-C-O and chi1-4 of one structure, no comparison) looped over the 64 structures
on the device, and metrics.sidechain_packing.  Per case: `call` = device events around REPS back-to-back calls of the Python function
(host overhead included), `graph` = the same calls captured once as a graph and replayed (device time per call; HIP only).  Prints one JSON
line.  Usage: python tools/eval_bench.py [--reps 200] [--only violations|sasa|torsions]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402
import dssp_build  # noqa: E402
import dssp_oracle  # noqa: E402
import sasa_oracle  # noqa: E402
import tm_oracle  # noqa: E402
import tmalign_oracle  # noqa: E402


def torch_pairwise(x, m, pairs):
    """proper Kabsch RMSD of the pairs (i, j) on mx[i] & mx[j], torch ops + batched torch.linalg.svd"""
    i, j = pairs[:, 0].long(), pairs[:, 1].long()
    a, b = x[i], x[j]
    w = (m[i] & m[j]).float()[..., None]
    n = w.sum(1, keepdim=True)
    a = a - (a * w).sum(1, keepdim=True) / n
    b = b - (b * w).sum(1, keepdim=True) / n
    s = (a * w).transpose(1, 2) @ b
    u, sig, vt = torch.linalg.svd(s)
    d = torch.sign(torch.linalg.det(u) * torch.linalg.det(vt))
    lam = sig[:, 0] + sig[:, 1] + d * sig[:, 2]
    e = ((a * a * w).sum((1, 2)) + (b * b * w).sum((1, 2)) - 2 * lam).clamp_min(0)
    return torch.sqrt(e / n[:, 0, 0])


def torch_batch_align(p1, p2, mask):
    """the reference's rule r = V U^T per sample (masked atoms as weights), applied to every atom"""
    B = p1.shape[0]
    x, y, w = p1.reshape(B, -1, 3), p2.reshape(B, -1, 3), mask.reshape(B, -1, 1).float()
    n = w.sum(1, keepdim=True)
    xm, ym = (x * w).sum(1, keepdim=True) / n, (y * w).sum(1, keepdim=True) / n
    s = ((x - xm) * w).transpose(1, 2) @ (y - ym)
    u, _, vt = torch.linalg.svd(s)
    r = vt.transpose(1, 2) @ u.transpose(1, 2)
    t = ym - xm @ r.transpose(1, 2)
    return (x @ r.transpose(1, 2) + t).reshape(p1.shape)


def timed(fn, reps, graph=True):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    call = e0.elapsed_time(e1) * 1e3 / reps
    if not graph:                      # (torch.linalg.svd is not captured: its solver may synchronise with the host)
        return {"call_us": round(call, 2)}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with _capi.capture_guard(), torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return {"call_us": round(call, 2), "graph_us": round(e0.elapsed_time(e1) * 1e3 / reps, 2)}


def pocket_cas(n_complex, n_samples, seed, n=25):
    """n_complex x n_samples peptide CA sets of n residues (samples of one complex: the native plus 2 A noise)"""
    xs = []
    for c in range(n_complex):
        batch = synth.make_pocket_batch(1, max(60, n + 35), n, seed=seed + c)
        ca = batch["pos_heavyatom"][0, batch["generate_mask"][0], 1]
        g = torch.Generator().manual_seed(seed + c)
        xs.append(ca[None] + 2.0 * torch.randn(n_samples, n, 3, generator=g))
    return torch.cat(xs).cuda().contiguous()


def tm_case(x, y, m, pairs, reps, n_check):
    """pf_tm_score_fwd on the pair list, timed, and checked against the float64 oracle on the first n_check pairs"""
    ours = geometry.tm_score(x, y, m, m, pairs)["tm"].cpu().double().numpy()
    xs, ys, ms, pp = x.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy(), pairs.cpu().numpy()
    t0 = time.perf_counter()
    ref = np.array([tm_oracle.tm_score(xs[i], ys[j], ms[i], ms[j])["tm"] for i, j in pp[:n_check]])
    per_pair = (time.perf_counter() - t0) / n_check
    return {"pairs": int(pairs.shape[0]), "checked": n_check, "max_abs_diff_tm": float(np.abs(ours[:n_check] - ref).max()),
            "hip": timed(lambda: geometry.tm_score(x, y, m, m, pairs), reps),
            "oracle_cpu_ms_per_pair": round(per_pair * 1e3, 2)}


def tmalign_case(x, y, mx, my, pairs, reps, n_check):
    """pf_tm_align_fwd on the pair list (max_len = the longest chain, as structure_scores passes it), timed, and checked against
    the float64 oracle on n_check pairs spread over the list"""
    max_len = int(torch.maximum(mx.sum(1).max(), my.sum(1).max()))
    out = geometry.tm_align(x, y, mx, my, pairs, alignment=True, max_len=max_len)
    tm, y2x = out["tm"].cpu().double().numpy(), out["y2x"].cpu().numpy()
    xs, ys, mxs, mys, pp = x.cpu().numpy(), y.cpu().numpy(), mx.cpu().numpy(), my.cpu().numpy(), pairs.cpu().numpy()
    pick = np.linspace(0, len(pp) - 1, n_check).astype(int)
    t0 = time.perf_counter()
    ref = [tmalign_oracle.tm_align(xs[pp[q, 0]], ys[pp[q, 1]], mxs[pp[q, 0]], mys[pp[q, 1]]) for q in pick]
    per_pair = (time.perf_counter() - t0) / n_check
    return {"pairs": int(pairs.shape[0]), "N": int(x.shape[1]), "max_len": max_len, "checked": n_check,
            "max_abs_diff_tm": float(max(abs(tm[q] - r["tm"]) for q, r in zip(pick, ref))),
            "map_mismatches": int(sum(not np.array_equal(y2x[q], r["y2x"]) for q, r in zip(pick, ref))),
            "hip": timed(lambda: geometry.tm_align(x, y, mx, my, pairs, max_len=max_len), reps),
            "oracle_cpu_ms_per_pair": round(per_pair * 1e3, 1)}


def dssp_chains(n_native, n_samples, n, seed):
    """n_native NeRF chains of n residues (phi / psi per segment from the helix, strand and coil basins), each repeated n_samples
    times with 0.3 A of noise -> pos [n_native * n_samples, n, 4, 3] on the device"""
    rng = np.random.default_rng(seed)
    nat = np.stack([dssp_build.random_chain(rng, n) for _ in range(n_native)])
    pos = nat[:, None] + 0.3 * rng.standard_normal((n_native, n_samples, n, 4, 3))
    return torch.from_numpy(pos.reshape(-1, n, 4, 3).astype(np.float32)).cuda()


def dssp_case(pos, reps, n_check):
    """pf_dssp_fwd on all chains, timed, and checked against the float64 oracle on the first n_check chains"""
    mask = torch.ones(pos.shape[:2], dtype=torch.bool, device=pos.device)
    ss = geometry.dssp(pos, mask).cpu().numpy()
    host = pos.cpu().double().numpy()
    t0 = time.perf_counter()
    ref = [dssp_oracle.dssp(host[b], np.ones(pos.shape[1], bool)) for b in range(n_check)]
    per_chain = (time.perf_counter() - t0) / n_check
    return {"chains": int(pos.shape[0]), "residues": int(pos.shape[1]), "checked": n_check,
            "mismatched": int(sum(not np.array_equal(ss[b], r["ss"]) for b, r in enumerate(ref))),
            "hip": timed(lambda: geometry.dssp(pos, mask), reps), "oracle_cpu_ms_per_chain": round(per_chain * 1e3, 3)}


def torch_dense_clashes(pos, exists, radius, index, tol=1.5):
    """the clash pass written densely with torch ops, pair tensors [B,L,L,14,14] -> per-atom loss, per-atom flag, mean loss [B]"""
    pos, exists = pos[:, :, :14], exists[:, :, :14]
    d = torch.sqrt(1e-10 + ((pos[:, :, None, :, None] - pos[:, None, :, None, :]) ** 2).sum(-1))
    m = exists[:, :, None, :, None] & exists[:, None, :, None, :] & (index[:, :, None] != index[:, None, :])[..., None, None]
    s = torch.arange(14, device=pos.device)
    cn = (index[:, :, None] + 1 == index[:, None, :])[..., None, None] & (s == 2)[:, None] & (s == 0)[None, :]
    m = m & ~cn & ~cn.permute(0, 2, 1, 4, 3) & ~((s == 5)[:, None] & (s == 5)[None, :])
    lim = radius[:, :, None, :, None] + radius[:, None, :, None, :] - tol
    e = torch.where(m, torch.relu(lim - d), torch.zeros_like(d))
    return e.sum((2, 4)), (m & (d < lim)).any(4).any(2), 0.5 * e.sum((1, 2, 3, 4)) / (1e-6 + 0.5 * m.sum((1, 2, 3, 4)))


def violation_cases(reps):
    out = {}
    table = geometry.vdw_radius_table().cuda()
    for L in (144, 512):
        batch = {k: v.cuda() for k, v in synth.make_pocket_batch(64, L, 12, seed=500 + L).items()}
        pos, mask, aa = batch["pos_heavyatom"], batch["mask_heavyatom"].to(torch.uint8), batch["aa"]
        index = metrics.residue_index(batch["chain_nb"], batch["res_nb"], batch["res_mask"])
        gen = batch["generate_mask"].to(torch.uint8)
        v = geometry.structural_violations(pos, mask, aa, index, group=gen)
        case = {"atoms": int(mask[:, :, :14].sum()), "atom_pairs_counted": int(v["clash_atom_pairs"].long().sum() // 2),
                "clashing_atoms": int(v["clash_atom"].sum()),
                "all_pairs": timed(lambda: geometry.structural_violations(pos, mask, aa, index), reps),
                "all_pairs_group": timed(lambda: geometry.structural_violations(pos, mask, aa, index, group=gen), reps),
                "query_generated": timed(lambda: geometry.structural_violations(pos, mask, aa, index, query=gen, group=gen), reps)}
        if L == 144:
            p8, m8, i8 = pos[:8], mask[:8].bool(), index[:8]
            r8 = table[aa[:8].clamp(0, 20)] * m8[:, :, :14]
            loss, flag, mean = torch_dense_clashes(p8, m8 & (torch.nn.functional.pad(table, (0, 1))[aa[:8].clamp(0, 20)] > 0), r8, i8)
            case["dense_torch_8x144"] = {"max_abs_diff_loss": float((loss - v["clash_atom_loss"][:8]).abs().max()),
                                         "flag_mismatches": int((flag != v["clash_atom"][:8]).sum()),
                                         "max_abs_diff_mean": float((mean - v["clash_mean_loss"][:8]).abs().max()),
                                         "hip_8x144": timed(lambda: geometry.structural_violations(p8, mask[:8], aa[:8], i8), reps),
                                         "torch": timed(lambda: torch_dense_clashes(p8, m8, r8, i8), max(reps // 20, 3), graph=False)}
            rot = torch.linalg.qr(torch.randn(64, L, 3, 3, generator=torch.Generator().manual_seed(505)))[0].cuda()
            final = {"rotmats": rot, "trans": pos[:, :, 1].contiguous(), "angles": batch["torsion_angle"], "seqs": aa, "seqs_1": aa}
            for bb in ("full_atom", "frames"):
                case[f"metrics_{bb}"] = timed(lambda: metrics.structural_violations(final, batch, backbone=bb), max(reps // 4, 3), graph=False)
        out[f"violations_64x{L}"] = case
    return out


def torch_chunked_sasa(pos, exists, R, u, chunk=8):
    """Shrake-Rupley with torch ops on the device: per sample the existing atoms, `chunk` atoms at a time against all of them
    ([chunk, P, atoms, 3] tensors) -> accessible points [B,N,15] int32"""
    B, N, S = exists.shape
    P = u.shape[0]
    count = torch.zeros(B, N, S, dtype=torch.int32, device=pos.device)
    for b in range(B):
        x, r = pos[b, :, :S][exists[b]], R[b][exists[b]]
        ids = torch.arange(x.shape[0], device=pos.device)
        acc = []
        for c0 in range(0, x.shape[0], chunk):
            xa, ra = x[c0:c0 + chunk], r[c0:c0 + chunk]
            t = (xa[:, None, :] - x[None])[:, None] + (ra[:, None, None] * u[None])[:, :, None]
            hit = ((t * t).sum(-1) < (r * r)[None, None, :]) & (ids[None, None, :] != ids[c0:c0 + chunk, None, None])
            acc.append(P - hit.any(-1).sum(-1))
        if acc:
            count[b][exists[b]] = torch.cat(acc).to(torch.int32)
    return count


def sasa_cases(reps):
    out = {}
    table = geometry.sasa_radius_table().cuda()
    for L in (144, 512):
        batch = {k: v.cuda() for k, v in synth.make_pocket_batch(64, L, 12, seed=600 + L).items()}
        pos, mask, aa = batch["pos_heavyatom"], batch["mask_heavyatom"].to(torch.uint8), batch["aa"]
        gen = batch["generate_mask"].to(torch.uint8)
        v = geometry.sasa(pos, mask, aa, group=gen)
        exists = mask.bool() & (table[aa.clamp(0, 20)] > 0)
        case = {"atoms": int(exists.sum()), "accessible_share": round(float(v["count"].sum()) / (960.0 * int(exists.sum())), 4),
                "mean_total_A2": round(float(v["sasa_total"].mean()), 1),
                "mean_buried_A2": round(float((v["sasa_total_own"] - v["sasa_total"]).mean()), 1)}
        for P in (960, 92):
            case[f"p{P}"] = timed(lambda: geometry.sasa(pos, mask, aa, n_points=P), reps)
            case[f"p{P}_group"] = timed(lambda: geometry.sasa(pos, mask, aa, group=gen, n_points=P), reps)
        case["p960_query_generated"] = timed(lambda: geometry.sasa(pos, mask, aa, query=gen, group=gen), reps)
        if L == 144:
            u = geometry.sphere_points(960).cuda()
            R = table[aa[:8].clamp(0, 20)] + 1.4
            dense = lambda: torch_chunked_sasa(pos[:8], exists[:8], R, u)  # noqa: E731
            diff = (dense() - v["count"][:8]).abs()
            case["chunked_torch_8x144"] = {"atoms_with_another_count": int((diff > 0).sum()), "max_abs_diff_count": int(diff.max()),
                                           "hip_8x144": timed(lambda: geometry.sasa(pos[:8], mask[:8], aa[:8]), reps),
                                           "torch": timed(dense, 3, graph=False)}
            t0 = time.perf_counter()
            o = sasa_oracle.sasa(pos[0].cpu().numpy(), mask[0].cpu().numpy(), aa[0].cpu().numpy(), table.cpu().numpy(), u.cpu().numpy())
            case["oracle_cpu_s_per_complex"] = round(time.perf_counter() - t0, 2)
            d0 = np.abs(o["count"] - v["count"][0].cpu().numpy())
            case["oracle_atoms_with_another_count"] = int((d0 > o["marginal"]).sum())
            rot = torch.linalg.qr(torch.randn(64, L, 3, 3, generator=torch.Generator().manual_seed(605)))[0].cuda()
            final = {"rotmats": rot, "trans": pos[:, :, 1].contiguous(), "angles": batch["torsion_angle"], "seqs": aa, "seqs_1": aa}
            for bb in ("full_atom", "frames"):
                case[f"interface_area_{bb}"] = timed(lambda: metrics.interface_area(final, batch, backbone=bb), max(reps // 4, 3), graph=False)
        out[f"sasa_64x{L}"] = case
    return out


def torsion_cases(reps):
    from pepflowww_amd.preprocess import get_torsion_angle
    B, L = 64, 144
    batch = {k: v.cuda() for k, v in synth.make_pocket_batch(B, L, 12, seed=744).items()}
    pos, mask, aa = batch["pos_heavyatom"], batch["mask_heavyatom"].to(torch.uint8), batch["aa"]
    index = metrics.residue_index(batch["chain_nb"], batch["res_nb"], batch["res_mask"])
    pos2 = (pos + 0.3 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(745)).cuda()).contiguous()
    ids = torch.arange(B, dtype=torch.int32, device="cuda")
    diag = torch.stack([ids, ids], 1)

    def side(p):
        t = geometry.torsion_angles(p, mask, aa, index)
        return dict(pos=p, atom_mask=mask, aa=aa, angles=t["angles"], defined=t["defined"])

    x, y = side(pos2), side(pos)
    both = lambda: geometry.sidechain_compare(side(pos2), side(pos), diag)  # noqa: E731
    c = both()
    case = {"angles_defined": int(y["defined"].sum()), "chi_compared": int(c["err_count"][:, 4:].sum()),
            "angles_one_structure": timed(lambda: geometry.torsion_angles(pos, mask, aa, index), reps),
            "compare_diagonal": timed(lambda: geometry.sidechain_compare(x, y, diag), reps),
            "compare_diagonal_per_residue": timed(lambda: geometry.sidechain_compare(x, y, diag, per_residue=True), reps),
            "angles_x2_and_compare": timed(both, reps),
            "torch_get_torsion_angle_x64": timed(lambda: [get_torsion_angle(pos[b], aa[b]) for b in range(B)], max(reps // 20, 3), graph=False)}
    ref = torch.stack([get_torsion_angle(pos[b], aa[b])[0] for b in range(B)])
    d = (y["angles"][:, :, 3:] - ref).abs()
    d = torch.minimum(d, 2 * np.pi - d)[y["defined"][:, :, 3:]]
    case["median_abs_diff_to_torch_rad"] = float(d.median())
    rot = torch.linalg.qr(torch.randn(B, L, 3, 3, generator=torch.Generator().manual_seed(746)))[0].cuda()
    final = {"rotmats": rot, "trans": pos[:, :, 1].contiguous(), "angles": batch["torsion_angle"], "seqs": aa, "seqs_1": aa}
    case["sidechain_packing"] = timed(lambda: metrics.sidechain_packing(final, batch), max(reps // 4, 3), graph=False)
    return {"torsions_64x144": case}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", choices=["violations", "sasa", "torsions"], default=None, help="run one leg alone")
    args = ap.parse_args()
    _capi.load()
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0)}
    if args.only in ("violations", "sasa", "torsions"):
        out.update({"violations": violation_cases, "sasa": sasa_cases, "torsions": torsion_cases}[args.only](args.reps))
        print(json.dumps(out))
        return
    for name, G in (("pairwise_64x25", 1), ("pairwise_16x64x25", 16)):
        x = pocket_cas(G, 64, 100)
        m = torch.ones(x.shape[:2], dtype=torch.bool, device=dev)
        pairs, _, _ = geometry.group_pairs(torch.arange(G).repeat_interleave(64))
        pairs = pairs.to(dev)
        ours = geometry.superpose(x, x, m, m, pairs)["rmsd"]
        ref = torch_pairwise(x, m, pairs)
        out[name] = {"pairs": int(pairs.shape[0]), "max_abs_diff_A": float((ours - ref).abs().max()),
                     "hip": timed(lambda: geometry.superpose(x, x, m, m, pairs), args.reps),
                     "torch_svd": timed(lambda: torch_pairwise(x, m, pairs), max(args.reps // 10, 5), graph=False)}
    B, L, A = 64, 128, 15
    batch = synth.make_pocket_batch(B, L, 20, seed=7)
    p2 = batch["pos_heavyatom"].cuda()
    mask = batch["mask_heavyatom"].cuda()
    p1 = (p2 + 1.5 * torch.randn(p2.shape, generator=torch.Generator().manual_seed(3)).cuda()).contiguous()
    ours = geometry.batch_align(p1, p2, mask)[0]
    ref = torch_batch_align(p1, p2, mask)
    out["batch_align_64x128x15"] = {"max_abs_diff_A": float((ours - ref).abs().max()),
                                    "hip": timed(lambda: geometry.batch_align(p1, p2, mask), args.reps),
                                    "torch_svd": timed(lambda: torch_batch_align(p1, p2, mask), max(args.reps // 10, 5), graph=False)}
    for name, n, G in (("tm_pairwise_64x15", 15, 1), ("tm_pairwise_64x25", 25, 1), ("tm_pairwise_16x64x25", 25, 16)):
        x = pocket_cas(G, 64, 200, n)
        m = torch.ones(x.shape[:2], dtype=torch.bool, device=dev)
        pairs, _, _ = geometry.group_pairs(torch.arange(G).repeat_interleave(64))
        out[name] = tm_case(x, x, m, pairs.to(dev), args.reps, 64)
    native = pocket_cas(1, 1, 300, 128).expand(64, 128, 3)
    sample = (native + 1.5 * torch.randn(native.shape, generator=torch.Generator().manual_seed(5)).cuda()).contiguous()
    ids = torch.arange(64, dtype=torch.int32, device=dev)
    out["tm_native_64x128"] = tm_case(sample, native.contiguous(), torch.ones(64, 128, dtype=torch.bool, device=dev),
                                      torch.stack([ids, ids], 1), args.reps, 8)
    ta_reps = max(args.reps // 10, 5)
    for name, G in (("tmalign_pairwise_64x25", 1), ("tmalign_pairwise_16x64x25", 16)):
        x = pocket_cas(G, 64, 200, 25)
        m = torch.ones(x.shape[:2], dtype=torch.bool, device=dev)
        pairs, _, _ = geometry.group_pairs(torch.arange(G).repeat_interleave(64))
        out[name] = tmalign_case(x, x, m, m, pairs.to(dev), ta_reps, 16)
    x25 = pocket_cas(1, 64, 200, 25)
    cplx = torch.randn(64, 128, 3, generator=torch.Generator().manual_seed(6)).cuda() * 10.0
    cplx[:, 40:65] = x25
    m = torch.zeros(64, 128, dtype=torch.bool, device=dev)
    m[:, 40:65] = True
    pairs, _, _ = geometry.group_pairs(torch.zeros(64, dtype=torch.int64))
    out["tmalign_pairwise_64x25_in128"] = tmalign_case(cplx, cplx, m, m, pairs.to(dev), ta_reps, 8)
    keep = torch.rand(64, 128, generator=torch.Generator().manual_seed(7)).cuda() > 0.15
    out["tmalign_native_64x128"] = tmalign_case(sample, native.contiguous(), keep,
                                                torch.ones(64, 128, dtype=torch.bool, device=dev), torch.stack([ids, ids], 1),
                                                ta_reps, 4)
    out["dssp_4096x25"] = dssp_case(dssp_chains(64, 64, 25, 400), args.reps, 64)
    out["dssp_64x128"] = dssp_case(dssp_chains(64, 1, 128, 401), args.reps, 16)
    out["dssp_8x512"] = dssp_case(dssp_chains(8, 1, 512, 402), args.reps, 4)
    batch = {k: v.cuda() for k, v in synth.make_pocket_batch(64, 60, 25, seed=403).items()}
    rot = torch.linalg.qr(torch.randn(64, 60, 3, 3, generator=torch.Generator().manual_seed(404)))[0].cuda()
    final = {"rotmats": rot, "trans": batch["pos_heavyatom"][:, :, 1].contiguous(), "angles": batch["torsion_angle"],
             "seqs": batch["aa"], "seqs_1": batch["aa"]}
    for bb in ("full_atom", "frames"):
        out[f"secondary_structure_64x25_{bb}"] = {"hip": timed(lambda: metrics.secondary_structure(final, batch, backbone=bb),
                                                               args.reps, graph=False)}
    out.update(violation_cases(args.reps))
    out.update(sasa_cases(args.reps))
    out.update(torsion_cases(args.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
