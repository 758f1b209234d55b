"""GPU checks of the point-mutation scan, pf_mutation_scan_fwd (geometry.mutation_scan), against the numpy float64 oracle
(scan_oracle.py): the energies and argmins of every candidate type on both sides of the 16-residue environment tile; a caller's
rotamer table on the edges of the kernel's row tile; bit-equality with pf_pack_sidechains_fwd on mutated inputs; hand-made cases;
energy_interface; bitwise repeatability and independence of the batch, of the other positions and of the other candidates; peak memory;
empty batches; metrics.mutation_scan after a short sample() run.  The comparison rule is pack_cases.bound, unchanged (scan_cases.py).
The scan is the packer's self energy on an unmoved environment: it is not FoldX and not Rosetta."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import pack_cases as PC  # noqa: E402
import pack_oracle as PO  # noqa: E402
import scan_cases as SC  # noqa: E402
import scan_oracle as SO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import mutation_scan as _is_there  # noqa: E402,F401
from test_gpu_pack import within  # noqa: E402

KEYS = SC.KEYS
OUT_BITS = ("scanned", "energy", "rotamer", "n_rotamers", "chi", "energy_interface", "ddE", "ddE_interface")


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def run(case, **kw):
    if "group" in case and "group" not in kw:
        kw["group"] = cu(case["group"])
    out = geometry.mutation_scan(*[cu(case[k]) for k in KEYS], **kw)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(out):
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v) for k, v in out.items()}


def check_against_oracle(case, oracles, got, chi_tab, M):
    """every output of the device against the oracle's; -> the largest |energy - oracle| / bound"""
    worst = 0.0
    B, N = case["aa"].shape
    assert got["energy"].shape == (B, N, 20) and got["chi"].shape == (B, N, 20, 4) and got["scanned"].dtype == np.bool_
    for b, o in enumerate(oracles):
        assert np.array_equal(got["scanned"][b], o.scanned), b
        done = np.zeros((N, 20), bool)
        for (q, t), z in o.res.items():
            done[q, t] = True
            bnd = SC.bound(z, M)
            r = int(got["rotamer"][b, q, t])
            assert 0 <= r < len(z["E"]) == got["n_rotamers"][b, q, t], (b, q, t, r)
            err = abs(float(got["energy"][b, q, t]) - z["E"][r])
            assert err <= bnd[r], (b, q, t, r, err, bnd[r])
            assert within(z["E"], r, bnd), (b, q, t, r, z["E"][r], z["E"].min())
            assert np.array_equal(got["chi"][b, q, t].view(np.int32), np.asarray(chi_tab[t, r], np.float32).view(np.int32)), (b, q, t)
            zi = dict(z["interface"], table=0.0)
            bi = SC.bound(zi, M)
            assert abs(float(got["energy_interface"][b, q, t]) - z["Ei"][r]) <= bi[r], (b, q, t, r)
            worst = max(worst, err / bnd[r]) if bnd[r] > 0 else worst
        assert np.isposinf(got["energy"][b][~done]).all() and np.isposinf(got["energy_interface"][b][~done]).all(), b
        assert (got["rotamer"][b][~done] == -1).all() and not got["n_rotamers"][b][~done].any() and not got["chi"][b][~done].any(), b
        assert np.isfinite(got["energy"][b][done]).all() and np.array_equal(np.isnan(got["ddE"][b]), ~done), b
        wt = np.clip(case["aa"][b], 0, 19)
        assert not got["ddE"][b][o.scanned, wt[o.scanned]].any() and not got["ddE_interface"][b][o.scanned, wt[o.scanned]].any()
    return worst


# ---- values ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", list(SC.SEEDS))
def test_values_against_the_oracle(N):
    case = SC.make_case(N)
    oracles, M = SC.oracle(case, key=N), SC.max_coord(case)        # the cap on near pairs is asserted here, before the device runs
    got = host(run(case))
    if N >= 6:
        assert oracles[1].scanned.sum() >= 0.6 * N and not oracles[2].scanned.any()       # every residue a position; none
    worst = check_against_oracle(case, oracles, got, PO.rotamer_table()[0], M)
    ala, gly = PO.res_index()["ALA"], PO.res_index()["GLY"]
    for b, o in enumerate(oracles):                         # no rotamer atom: the table's energy, 0
        assert not got["energy"][b][o.scanned][:, [ala, gly]].any()
    print(f"N = {N}: largest |energy - oracle| / bound = {worst:.3f}")


def test_rotamer_tile_edges():
    """a caller's table: rows (count x the type's atoms) one below, at and one above the multiples of the kernel's 256-row pass, counts
    63, 64, 65 around a wave of the argmin, counts 1 and 128; random table energies"""
    case, table = SC.edge_case(), SC.edge_table()
    oracles, M = SC.oracle(case, key="edge", rotamers=table), SC.max_coord(case)
    got = host(run(case, rotamers=tuple(torch.from_numpy(v) for v in table)))
    worst = check_against_oracle(case, oracles, got, table[0], M)
    idx = PO.res_index()
    for b, o in enumerate(oracles):
        q = int(np.flatnonzero(o.scanned)[0])
        assert got["n_rotamers"][b, q, idx["CYS"]] == 128 and got["n_rotamers"][b, q, idx["SER"]] == 1
        assert got["energy"][b, q, idx["ALA"]] == table[2][idx["ALA"], 0]                      # no atoms: the table energy alone
        assert got["energy"][b, q, idx["GLY"]] == table[2][idx["GLY"], :3].min()
    print(f"tile edges: largest |energy - oracle| / bound = {worst:.3f}")


# ---- against pf_pack_sidechains_fwd, bitwise -----------------------------------------------------------------------------------------

def test_bitwise_equal_to_pack_sidechains_on_mutated_inputs():
    """N = 17, every candidate type at 3 positions of every structure that has them: energy[b,q,t] and rotamer[b,q,t] are
    energy_self_best[b,q] and rotamer[b,q] of pack_sidechains(aa with aa[q] := t, movable = onehot(q), sweeps=0), as int32 bit
    patterns: the same build, the same pairs, the same order of every sum"""
    case = SC.make_case(17)
    B, N = case["aa"].shape
    got = run(case)
    scanned = got["scanned"].cpu().numpy()
    picks = np.full((B, 3), -1)
    for b in range(B):
        qs = np.flatnonzero(scanned[b])
        if len(qs) >= 3:
            picks[b] = qs[[0, len(qs) // 2, -1]]
    rows = np.flatnonzero(picks[:, 0] >= 0)
    assert len(rows) >= 2
    pos, mask, idx = (cu(case[k][rows]) for k in ("pos", "atom_mask", "residue_index"))
    e_bits, checked = got["energy"].view(torch.int32), 0
    for k in range(3):
        q = torch.as_tensor(picks[rows, k]).cuda()
        movable = torch.zeros(len(rows), N, dtype=torch.bool, device="cuda")
        movable[torch.arange(len(rows)), q] = True
        for t in range(20):
            aa = cu(case["aa"][rows]).clone()
            aa[torch.arange(len(rows)), q] = t
            p = geometry.pack_sidechains(pos, mask, aa, idx, movable, sweeps=0)
            want_e = p["energy_self_best"][torch.arange(len(rows)), q].view(torch.int32)
            want_r = p["rotamer"][torch.arange(len(rows)), q]
            have_e = e_bits[torch.as_tensor(rows).cuda(), q, t]
            have_r = got["rotamer"][torch.as_tensor(rows).cuda(), q, t]
            assert torch.equal(have_e, want_e), (k, t, have_e.tolist(), want_e.tolist())
            assert torch.equal(have_r, want_r), (k, t)
            checked += len(rows)
    assert checked >= 120


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------

def test_hand_lone():
    idx = PO.res_index()
    for name in ("MET", "SER", "LEU"):
        case = SC.hand_lone(name)
        got = host(run(case))
        wt = idx[name]
        assert got["scanned"].tolist() == [[True]] and (got["rotamer"][0, 0] >= 0).all()
        assert got["ddE"][0, 0, wt] == 0.0 and got["ddE_interface"][0, 0, wt] == 0.0
        assert got["energy"][0, 0, idx["ALA"]] == 0.0 and got["energy"][0, 0, idx["GLY"]] == 0.0
        assert got["ddE"][0, 0, idx["ALA"]] == -got["energy"][0, 0, wt] == got["ddE"][0, 0, idx["GLY"]]
        assert not got["energy_interface"].any()            # nothing but its own residue
        o = SO.Scan(*[case[k][0] for k in KEYS])
        z = o.res[0, wt]
        r = int(got["rotamer"][0, 0, wt])
        assert abs(float(got["energy"][0, 0, wt]) - z["E"][r]) <= SC.bound(z, SC.max_coord(case))[r]
        # the packer's own start on the same residue
        p = geometry.pack_sidechains(*[cu(case[k]) for k in KEYS], sweeps=0)
        assert int(p["rotamer"][0, 0]) == r and float(p["energy_self_best"][0, 0]) == float(got["energy"][0, 0, wt])


def test_hand_pocket_larger_hydrophobic_gains_contacts():
    case, group = SC.hand_pocket()
    idx = PO.res_index()
    got = host(run(case, group=cu(group)))
    lone = host(run(SC.hand_lone("ALA")))
    M = SC.max_coord(case)
    o = SO.Scan(*[case[k][0] for k in KEYS], group=group[0], near=PC.pos_err(M))
    leu, ile, ala = idx["LEU"], idx["ILE"], idx["ALA"]
    want = o.res[0, leu]["E"].min()
    assert want < -0.5 and want < -100 * SC.bound(o.res[0, leu], M).max()                 # the oracle: eight contacts, far from 0
    assert got["ddE"][0, 0, ala] == 0.0                                                  # the wild type
    assert got["ddE"][0, 0, leu] < -0.5 and got["ddE"][0, 0, ile] < 0.0
    assert got["ddE"][0, 0, leu] < lone["ddE"][0, 0, leu] - 0.5                          # and it is the pocket that does it
    assert got["ddE_interface"][0, 0, leu] < -0.5
    assert (got["scanned"][0, 1:] == False).all() and np.isposinf(got["energy"][0, 1:]).all()  # noqa: E712


def test_hand_cys_adds_nothing_from_sg_sg():
    case = SC.hand_cys()
    idx = PO.res_index()
    got, lone = _bits(run(case)), _bits(run(SC.hand_lone("ALA")))
    cys, ser = idx["CYS"], idx["SER"]
    assert torch.equal(got["energy"][0, 0, cys], lone["energy"][0, 0, cys]) and torch.equal(got["rotamer"][0, 0, cys], lone["rotamer"][0, 0, cys])
    e, e0 = got["energy"].view(torch.float32), lone["energy"].view(torch.float32)
    assert float(e[0, 0, ser]) > float(e0[0, 0, ser]) + 0.5         # an OG there is inside the SG


def test_hand_pro_obeys_the_peptide_bond_exclusions():
    idx = PO.res_index()
    pro = idx["PRO"]
    res = {}
    for bonded in (True, False):
        case = SC.hand_pro(bonded)
        M = SC.max_coord(case)
        got = run(case)
        o = SO.Scan(*[case[k][0] for k in KEYS], near=PC.pos_err(M))
        z = o.res[1, pro]
        r = int(got["rotamer"][0, 1, pro])
        assert abs(float(got["energy"][0, 1, pro]) - z["E"][r]) <= SC.bound(z, M)[r], bonded
        assert within(z["E"], r, SC.bound(z, M))
        res[bonded] = _bits(got)
    e = {k: v["energy"].view(torch.float32)[0, 1] for k, v in res.items()}
    assert float(e[True][pro]) < float(e[False][pro]) - 1.0         # CD against CA, C, O and CG against C: left out when bonded
    others = [t for t in range(20) if t != pro]
    assert torch.equal(res[True]["energy"][0, 1, others], res[False]["energy"][0, 1, others])


# ---- energy_interface ------------------------------------------------------------------------------------------------------------------

def test_energy_interface():
    """every other residue in another group (a group byte of its own each), no own-residue pair evaluated and a zero table energy:
    energy_interface is energy, bit for bit; one group: 0.  Own-residue pairs: with O and slot 14 masked off, the types whose
    rotamer atoms are all within three bonds of N, CA, C and CB and of each other have none (own_pair_table says which)."""
    case = SC.make_case(17)
    B, N = case["aa"].shape
    case["atom_mask"] = case["atom_mask"].copy()
    case["atom_mask"][:, :, [3, 14]] = False
    own = PO.own_pair_table()[:20].copy()
    own[:, :, [3, 14]] = False
    rows = SC.rows_of_type()
    bare = [t for t in range(20) if rows[t] > 0 and not own[t].any()]
    assert len(bare) >= 4, bare                             # SER, CYS, THR, VAL at least
    args = [cu(case[k]) for k in KEYS]
    each = np.broadcast_to(np.arange(N, dtype=np.uint8), (B, N)).copy()
    split = _bits(geometry.mutation_scan(*args, group=cu(each)))
    one = _bits(geometry.mutation_scan(*args, group=cu(np.ones((B, N), bool))))
    none = _bits(geometry.mutation_scan(*args))
    done = split["rotamer"] >= 0
    assert int(done[:, :, bare].sum()) >= 40
    assert torch.equal(split["energy_interface"][:, :, bare], split["energy"][:, :, bare])
    assert bool((split["energy"].view(torch.float32)[:, :, bare][done[:, :, bare]] != 0).any())
    assert not torch.equal(split["energy_interface"], split["energy"])         # (the other types have own-residue pairs)
    for r in (one, none):
        assert torch.equal(r["energy"], split["energy"]) and torch.equal(r["rotamer"], split["rotamer"])
        assert not r["energy_interface"][done].any() and bool(torch.isposinf(r["energy_interface"].view(torch.float32)[~done]).all())


# ---- repeatability and independence ----------------------------------------------------------------------------------------------------

def test_bitwise_repeatable_and_independent():
    case = SC.make_case(33)
    B, N = case["aa"].shape
    a, b = _bits(run(case)), _bits(run(case))
    perm = [2, 0, 3, 1]
    shuffled = _bits(run({k: v[perm].copy() for k, v in case.items()}))
    for k in OUT_BITS:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][perm], shuffled[k]), k
    one = _bits(run({k: v[1:2] for k, v in case.items()}))
    for k in OUT_BITS:
        assert torch.equal(a[k][1], one[k][0]), k
    # a subset of the positions: the same numbers there, the fill elsewhere
    sub = case["positions"].copy()
    sub[:, ::2] = False
    part = _bits(run(dict(case, positions=sub)))
    keep = cu(sub) & a["scanned"]
    assert int(keep.sum()) > 0 and torch.equal(part["scanned"], keep)
    for k in OUT_BITS[1:]:
        assert torch.equal(part[k][keep], a[k][keep]), k
    assert bool((part["rotamer"][~keep] == -1).all())
    # a subset of the candidates (one mask for all, and per residue): the same numbers there, the wild type always
    few = np.zeros(20, bool)
    few[[PO.res_index()[n] for n in ("ALA", "LEU", "ARG")]] = True
    wild = torch.nn.functional.one_hot(cu(case["aa"]).clamp(0, 19), 20).bool()
    per = np.random.default_rng(3).random((B, N, 20)) < 0.3
    for cand, mask in ((few, cu(few)[None, None, :]), (per, cu(per))):
        part = _bits(run(case, candidates=cu(cand)))
        on = (mask | wild) & a["scanned"][:, :, None]
        assert torch.equal(part["rotamer"] >= 0, on)
        for k in OUT_BITS[1:]:
            assert torch.equal(part[k][on], a[k][on]), k
        assert bool(torch.isposinf(part["energy"].view(torch.float32)[~on]).all())


# ---- memory, empty batches ---------------------------------------------------------------------------------------------------------

def test_peak_memory_is_the_outputs_and_the_workspace():
    """B = 4, N = 33: beyond its inputs the call holds its outputs, its workspace pf_mutation_scan_work_bytes(B, N) = 272 bytes per
    residue -- nothing per type or rotamer -- and, while ddE is formed, at most four more [B,N,20] temporaries of 4 bytes.  Slack: 64
    KiB for the allocator's rounding of each tensor to 512 bytes."""
    case = SC.make_case(33)
    B, N = case["aa"].shape
    args = [cu(case["pos"]), cu(case["atom_mask"]).view(torch.uint8), cu(case["aa"]), cu(case["residue_index"]),
            cu(case["positions"]).view(torch.uint8)]
    geometry.mutation_scan(*[t[:1] for t in args])          # the constant tables are on the device
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = geometry.mutation_scan(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    work = _capi.load().pf_mutation_scan_work_bytes(B, N)
    assert work == B * N * 272
    assert peak - base <= work + out_bytes + 4 * B * N * 20 * 4 + 64 * 1024, (peak - base, work, out_bytes)
    assert work < _capi.load().pf_pack_work_bytes(B, N, 108) // 50


def test_empty_batches_launch_nothing():
    for B, N in ((0, 5), (3, 0)):
        pos, mask = torch.zeros(B, N, 15, 3).cuda(), torch.ones(B, N, 15, dtype=torch.bool).cuda()
        aa, idx = torch.zeros(B, N, dtype=torch.int64).cuda(), torch.zeros(B, N, dtype=torch.int32).cuda()
        sel = torch.ones(B, N, dtype=torch.bool).cuda()
        calls = _capi.CALLS
        r = geometry.mutation_scan(pos, mask, aa, idx, sel, group=sel)
        assert _capi.CALLS == calls
        assert r["energy"].shape == (B, N, 20) and r["chi"].shape == (B, N, 20, 4) and r["ddE"].shape == (B, N, 20)
        assert r["scanned"].shape == (B, N) and r["scanned"].dtype == torch.bool and r["rotamer"].dtype == torch.int32


# ---- metrics.mutation_scan -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_mutation_scan_after_sample(model):
    B, L, NS, K = 4, 40, 3, 5
    batch = synth.make_pocket_batch(B, L, 12, seed=71)
    noise = synth.make_noise(B, L, NS, seed=72)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    gen = dev_batch["generate_mask"].bool() & dev_batch["res_mask"].bool()
    out = metrics.mutation_scan(final, dev_batch, top_k=K)
    ala = PO.res_index()["ALA"]
    assert out["ddE"].shape == (B, L, 20) and out["ddE"].dtype == torch.float32 and out["ddE_interface"].shape == (B, L, 20)
    assert out["ddE_ala"].shape == (B, L) and out["hot_spot"].shape == (B, L) and out["hot_spot"].dtype == torch.bool
    assert out["top_position"].shape == (B, K) and out["top_type"].shape == (B, K) and out["top_ddE"].shape == (B, K)
    nan_eq = lambda x, y: torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0))  # noqa: E731
    assert nan_eq(out["ddE_ala"], out["ddE"][:, :, ala])
    assert torch.equal(out["hot_spot"], out["ddE_ala"] >= metrics.HOT_SPOT_DDE)
    # nothing outside the generated residues is evaluated; inside, every type of every residue of a type in 0..19
    aa = torch.where(gen, cu(final["seqs"]), cu(final["seqs_1"]))
    want = gen & (aa < 20)
    assert torch.equal(out["scanned"], want) and torch.equal(out["rotamer"] >= 0, want[:, :, None].expand(B, L, 20))
    assert bool(torch.isnan(out["ddE"][~want]).all()) and bool(torch.isfinite(out["ddE"][want]).all())
    assert not torch.gather(out["ddE"], 2, aa.clamp(0, 19)[:, :, None])[want].any()
    # the top_k entries are the smallest ddE values, the wild type aside
    wild = torch.nn.functional.one_hot(aa.clamp(0, 19), 20).bool()
    flat = torch.where(torch.isnan(out["ddE"]) | wild, torch.full_like(out["ddE"], float("inf")), out["ddE"]).reshape(B, L * 20)
    smallest = torch.sort(flat, 1).values[:, :K]
    assert torch.equal(out["top_ddE"], smallest) and bool((out["top_ddE"][:, 1:] >= out["top_ddE"][:, :-1]).all())
    assert torch.equal(out["ddE"][torch.arange(B)[:, None], out["top_position"], out["top_type"]], out["top_ddE"])
    assert bool(gen[torch.arange(B)[:, None], out["top_position"]].all())
    # an alanine scan alone gives the same column; the complex is binding_energy's "packed" one
    only = metrics.mutation_scan(final, dev_batch, candidates="ALA", top_k=2)
    assert nan_eq(only["ddE_ala"], out["ddE_ala"])
    assert torch.equal(only["rotamer"] >= 0, want[:, :, None] & (wild | (torch.arange(20, device="cuda") == ala)))
    print("mutation_scan: hot spots per sample", out["hot_spot"].sum(1).tolist(), "best substitutions",
          [(int(p), int(t), round(float(v), 2)) for p, t, v in zip(out["top_position"][:, 0], out["top_type"][:, 0], out["top_ddE"][:, 0])])
