"""GPU checks of the rotamer side-chain packing, pf_pack_sidechains_fwd (geometry.pack_sidechains), against the numpy float64 oracle
(pack_oracle.py): the self energies and the start on the tile edges of a 16-residue tile; the search, replayed decision by decision from
the device's own states; the hand-computed cases; what the output keeps of its input; bitwise repeatability and independence of the
batch; peak memory; metrics.pack_samples and backbone="packed" after a short sample() run.  The comparison rule is derived in
pack_cases.py.  The packer is a staggered rotamer grid with this package's own pair energy: it is not SCWRL4 and not Rosetta's."""
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
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import pack_sidechains as _is_there  # noqa: E402,F401

KEYS = ("pos", "atom_mask", "aa", "residue_index", "movable")
SHAPES = {1: 6, 2: 6, 15: 6, 16: 6, 17: 6, 33: 4, 52: 4, 144: 2}


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def run(case, **kw):
    out = geometry.pack_sidechains(*[cu(case[k]) for k in KEYS], **kw)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(out):
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    return {k: (v.view(view[v.dtype]) if v.dtype in view else v) for k, v in out.items()}


def get_case(N):
    """the seeded case of N residues and its oracles (made once); N = 16 has 14 atom slots"""
    case = PC.make_case(100 + N, SHAPES[N], N, A=14 if N == 16 else 15)
    return case, PC.oracle(case, key=N), PC.max_coord(case)


def within(e, r_dev, bnd):
    """the decision rule: the oracle's energy of the device's choice against the oracle's minimum"""
    r_min = int(np.argmin(e))
    return e[r_dev] <= e[r_min] + 2.0 * max(bnd[r_dev], bnd[r_min])


# ---- self energy and start -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", list(SHAPES))
def test_self_energy_and_start(N):
    case, oracles, M = get_case(N)
    B = SHAPES[N]
    got = host(run(case, sweeps=0, trace=True))
    assert got["choice_trace"].shape == (B, 0, N) and got["energy_trace"].shape == (B, 1) and got["changed"].shape == (B, 0)
    assert not got["sweeps_run"].any()
    if N >= 6:
        assert oracles[1].packed.sum() >= 0.6 * N and (B < 3 or not oracles[2].packed.any())       # every residue movable; none
    worst = 0.0
    for b, o in enumerate(oracles):
        assert np.array_equal(got["packed"][b], o.packed), b
        assert np.array_equal(got["rotamer"][b] >= 0, o.packed) and (got["rotamer"][b][~o.packed] == -1).all()
        assert (got["n_rotamers"][b][o.plist] == np.asarray(o.count, np.int32)).all() and not got["n_rotamers"][b][~o.packed].any()
        assert not got["energy_self_best"][b][~o.packed].any() and not got["energy_residue"][b][~o.packed].any()
        start = []
        for p, q in enumerate(o.plist):
            s = o.self_[p]
            bnd = PC.bound(s, M)
            r = int(got["rotamer"][b, q])
            assert 0 <= r < o.count[p]
            err = abs(float(got["energy_self_best"][b, q]) - s["E"][r])
            assert err <= bnd[r], (b, q, r, err, bnd[r])
            assert within(s["E"], r, bnd), (b, q, r, s["E"][r], s["E"].min())
            worst = max(worst, err / bnd[r]) if bnd[r] > 0 else worst
            start.append(r)
        tot = o.total(start)
        assert abs(got["energy_trace"][b, 0] - tot["E"]) <= PC.bound(tot, M), (b, got["energy_trace"][b, 0], tot["E"])
    print(f"N = {N}: largest |E_self - oracle| / bound = {worst:.3f}")


# ---- the search, replayed ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,sweeps", [(17, 8), (52, 4), (144, 2)])
def test_replay(N, sweeps):
    case, oracles, M = get_case(N)
    B = SHAPES[N]
    first = host(run(case, sweeps=0))
    got = host(run(case, sweeps=sweeps, trace=True))
    assert got["choice_trace"].shape == (B, sweeps, N) and got["energy_trace"].shape == (B, sweeps + 1)
    assert np.array_equal(got["energy_self_best"], first["energy_self_best"]) and np.array_equal(got["energy_trace"][:, 0], first["energy_trace"][:, 0])
    late = 0
    for b, o in enumerate(oracles):
        cur = [int(first["rotamer"][b, q]) for q in o.plist]
        trace, run_n = got["energy_trace"][b], int(got["sweeps_run"][b])
        assert 0 < run_n <= sweeps
        for s in range(run_n):
            changed = 0
            for p, q in enumerate(o.plist):
                z = o.conditional(p, cur)
                r = int(got["choice_trace"][b, s, q])
                assert 0 <= r < o.count[p] and within(z["E"], r, PC.bound(z, M)), (b, s, q, r)
                changed += r != cur[p]
                cur[p] = r
            assert (got["choice_trace"][b, s][~o.packed] == -1).all()
            assert int(got["changed"][b, s]) == changed, (b, s)
            tot = o.total(cur)
            bnd = PC.bound(tot, M)
            assert abs(trace[s + 1] - tot["E"]) <= bnd, (b, s, trace[s + 1], tot["E"], bnd)
            assert trace[s + 1] <= trace[s] + bnd, (b, s)                   # never rises by more than the bound
            late += s > 0 and changed > 0
            assert (changed == 0) == (s == run_n - 1) or s == sweeps - 1
        # the sweeps that did not run
        assert (got["choice_trace"][b, run_n:] == -1).all() and not got["changed"][b, run_n:].any()
        assert (trace[run_n + 1:] == trace[run_n]).all()
        assert [int(got["rotamer"][b, q]) for q in o.plist] == cur
        # energy_residue: E_self plus half of each of the residue's pair terms at the end
        for p, q in enumerate(o.plist):
            z = o.conditional(p, cur)
            want = 0.5 * (z["E"][cur[p]] + o.self_[p]["E"][cur[p]])
            bnd = {k: (v[cur[p]] if np.ndim(v) else v) for k, v in z.items()}
            assert abs(float(got["energy_residue"][b, q]) - want) <= PC.bound(bnd, M), (b, q)
        pos, mask, chi = o.output(cur)
        assert np.array_equal(got["atom_mask"][b], mask)
        assert np.abs(got["pos"][b].astype(np.float64) - pos)[mask].max() <= PC.build_err(M)
        assert np.array_equal(got["chi"][b], chi.astype(np.float32))
    print(f"N = {N}: rotamers changed after the first sweep in {late} (structure, sweep) pairs")


def test_small_seeds_reach_the_brute_force_minimum():
    seeds = PC.small_seeds()
    cases = [PC.small_case(s) for s in seeds]
    got = host(run({k: np.concatenate([c[k] for c in cases]) for k in KEYS}, trace=True))
    for b, (s, case) in enumerate(zip(seeds, cases)):
        o = PO.Structure(*[case[k][0] for k in KEYS])
        run_o = o.icm(8)
        best, arg = o.brute_force()
        assert run_o["rotamer"] == arg
        assert abs(got["energy_trace"][b, -1] - best) <= PC.bound(o.total(arg), PC.max_coord(case)), s
        if PC.small_report(s)["clear"] == 1.0:              # every runner-up ten bounds away: the device walks the oracle's own path
            assert [int(got["rotamer"][b, q]) for q in o.plist] == arg, s
            n = run_o["sweeps_run"]
            assert int(got["sweeps_run"][b]) == n and got["changed"][b, :n].tolist() == run_o["changed"], s


# ---- hand-computed cases ---------------------------------------------------------------------------------------------------------------

def test_hand_ser():
    case, want, _ = PC.hand_ser()
    got = host(run(case))
    assert got["rotamer"][0].tolist() == [want, -1] and got["packed"][0].tolist() == [True, False]
    assert np.array_equal(got["pos"][0, 1], case["pos"][0, 1]) and np.array_equal(got["atom_mask"][0, 1], case["atom_mask"][0, 1])
    assert abs(np.degrees(got["chi"][0, 0, 0]) - 60.0) < 1e-4 and not got["chi"][0, 0, 1:].any()


def test_hand_leu():
    case = PC.hand_leu()
    start, got = host(run(case, sweeps=0)), host(run(case, trace=True))
    assert start["rotamer"][0].tolist() == [3, 3] and got["rotamer"][0].tolist() == [8, 8]
    assert int(got["sweeps_run"][0]) == 2 and got["changed"][0].tolist() == [2, 0] + [0] * 6
    assert got["choice_trace"][0, :2].tolist() == [[8, 8], [8, 8]] and (got["choice_trace"][0, 2:] == -1).all()
    trace = got["energy_trace"][0]
    assert trace[0] > 9.0 and trace[1] < 1.0 and (trace[1:] == trace[1]).all()
    o = PO.Structure(*[case[k][0] for k in KEYS])
    M = PC.max_coord(case)
    for cur, e in (([3, 3], trace[0]), ([8, 8], trace[-1])):
        tot = o.total(cur)
        assert abs(e - tot["E"]) <= PC.bound(tot, M)
    # the repulsion between the two side chains, from the device's coordinates: there at the start, gone at the end
    overlap = []
    for out in (start, got):
        a, b = out["pos"][0, 0, 5:8].astype(np.float64), out["pos"][0, 1, 5:8].astype(np.float64)
        d = np.sqrt(((a[:, None] - b[None]) ** 2).sum(-1)) - 3.8
        overlap.append(float(np.clip(-d, 0, None).max()))
    assert overlap[0] > 1.0 and overlap[1] == 0.0


def test_hand_lone():
    case = PC.hand_lone("MET")
    o = PO.Structure(*[case[k][0] for k in KEYS])
    want = int(np.argmin(o.self_[0]["E"]))
    got = host(run(case))
    assert got["rotamer"][0, 0] == want and int(got["sweeps_run"][0]) == 1 and not got["changed"].any()
    assert abs(float(got["energy_self_best"][0, 0]) - o.self_[0]["E"][want]) <= PC.bound(o.self_[0], PC.max_coord(case))[want]
    assert got["energy_residue"][0, 0] == got["energy_self_best"][0, 0] and (got["energy_trace"][0] == got["energy_trace"][0, 0]).all()
    assert np.array_equal(got["pos"][0, 0, :4], case["pos"][0, 0, :4])
    chi_t, count, energy = geometry.rotamer_table()
    energy = energy.clone()
    energy[o.t[0], 5] = -50.0
    assert host(run(case, rotamers=(chi_t, count, energy)))["rotamer"][0, 0] == 5


# ---- what the output keeps -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [16, 33])
def test_output_invariants(N):
    case, oracles, _ = get_case(N)
    A = case["pos"].shape[2]
    out = run(case, sweeps=2)
    got = host(out)
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.int32)  # noqa: E731
    mask_tab = PO.rigid()["mask"]
    n_packed = 0
    for b, o in enumerate(oracles):
        keep = [0, 1, 2, 3] + ([14] if A > 14 else [])
        assert np.array_equal(bits(got["pos"][b][:, keep]), bits(case["pos"][b][:, keep])), b      # N, CA, C, O, slot 14
        assert np.array_equal(got["atom_mask"][b][:, keep], case["atom_mask"][b][:, keep]), b
        un = ~o.packed
        assert np.array_equal(bits(got["pos"][b][un][:, :A]), bits(case["pos"][b][un])), b          # every atom of an unpacked residue
        assert np.array_equal(got["atom_mask"][b][un][:, :A], case["atom_mask"][b][un]), b
        if A == 14:
            assert not got["atom_mask"][b][:, 14].any() and not got["pos"][b][:, 14].any()
        assert np.array_equal(got["atom_mask"][b][o.packed][:, 4:14], mask_tab[o.t[o.packed]][:, 4:14]), b        # the type's mask
        n_packed += int(o.packed.sum())
    assert n_packed > 0


def _chi_errors(case, out):
    """|chi measured by geometry.torsion_angles on the packed structure - the chosen rotamer's chi| (mod 2 pi) where the type has
    the chi and the residue is packed -> [n,4] (NaN elsewhere)"""
    t = geometry.torsion_angles(out["pos"], out["atom_mask"], cu(case["aa"]), cu(case["residue_index"]))
    d = (t["angles"][:, :, 4:] - out["chi"]).double()
    d = (torch.remainder(d + np.pi, 2 * np.pi) - np.pi).abs()
    has = (geometry.chi_atom_table()[:, :, 0] >= 0).cuda()[cu(case["aa"]).clamp(0, 20)] & out["packed"][:, :, None]
    assert bool((t["defined"][:, :, 4:] | ~has).all())
    return torch.where(has, d, torch.full_like(d, float("nan")))[out["packed"]].cpu().numpy()


def test_output_chi_on_ideal_backbones():
    """all 20 types on the rigid-group table's own backbones: torsion_angles gives back every chi of the chosen rotamer to 1e-4"""
    case = PC.ideal_case()
    err = _chi_errors(case, run(case))
    assert np.nanmax(err) <= 1e-4, np.nanmax(err, 0)


@pytest.mark.parametrize("N", [16, 33])
def test_output_chi_matches_torsion_angles(N):
    """geometry.torsion_angles of the output gives `chi` (mod 2 pi) to 1e-4 rad on the seeded NeRF backbones, whose N-CA-C angle
    (111.2 degrees) is off every type's ideal: chi1 is measured from the real N, and the kernel turns the first frame by chi1 minus
    the angle between the real and the ideal N about CA-CB.  (Without that correction chi1 was off by 2.39e-2 rad here.)"""
    case, _, _ = get_case(N)
    err = _chi_errors(case, run(case, sweeps=2))
    worst = np.nanmax(err, 0)
    print(f"N = {N}: largest |measured - chi| per chi = {worst}")
    assert (worst <= 1e-4).all(), worst


# ---- repeatability -----------------------------------------------------------------------------------------------------------------

def test_bitwise_repeatable_and_independent_of_batch_and_order():
    case, _, _ = get_case(52)
    B = SHAPES[52]
    a, b = _bits(run(case, sweeps=3, trace=True)), _bits(run(case, sweeps=3, trace=True))
    perm = [2, 0, 3, 1]
    shuffled = _bits(run({k: v[perm].copy() for k, v in case.items()}, sweeps=3, trace=True))
    assert bool(a["changed"].any())
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][perm], shuffled[k]), k
    for i in range(B):
        one = _bits(run({k: v[i:i + 1] for k, v in case.items()}, sweeps=3, trace=True))
        for k in a:
            assert torch.equal(a[k][i], one[k][0]), (i, k)


# ---- memory, empty batches ---------------------------------------------------------------------------------------------------------

def test_peak_memory_is_the_workspace():
    """B = 2, N = 144: beyond its inputs and outputs the call holds its workspace, pf_pack_work_bytes(B, N, 108), and nothing else.
    Slack: 64 KiB for the allocator's rounding of each of the 13 tensors to 512 bytes and for the argument struct's tables (already on
    the device after the first call, so 0)."""
    case, _, _ = get_case(144)
    B, N = 2, 144
    args = [cu(case["pos"]), cu(case["atom_mask"]).view(torch.uint8), cu(case["aa"]), cu(case["residue_index"]),
            cu(case["movable"]).view(torch.uint8)]
    geometry.pack_sidechains(*[t[:1] for t in args], sweeps=1)          # the constant tables are on the device
    torch.cuda.synchronize()
    # device tensors of earlier tests that only the cyclic collector frees are freed here, so that the allocator state the
    # measurement starts from does not depend on where in the session the collector last ran (a cached block up to 1 MiB larger
    # than the request is handed out whole and counts as allocated)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = geometry.pack_sidechains(*args, sweeps=2, trace=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    work = _capi.load().pf_pack_work_bytes(B, N, 108)
    assert work == B * N * (288 + 148 * 108)
    assert peak - base <= work + out_bytes + 64 * 1024, (peak - base, work, out_bytes)


def test_empty_batches_launch_nothing():
    for B, N in ((0, 5), (3, 0)):
        pos, mask = torch.zeros(B, N, 15, 3).cuda(), torch.ones(B, N, 15, dtype=torch.bool).cuda()
        aa, idx = torch.zeros(B, N, dtype=torch.int64).cuda(), torch.zeros(B, N, dtype=torch.int32).cuda()
        mov = torch.ones(B, N, dtype=torch.bool).cuda()
        r = geometry.pack_sidechains(pos, mask, aa, idx, mov, sweeps=3, trace=True)
        assert r["pos"].shape == (B, N, 15, 3) and r["energy_trace"].shape == (B, 4) and not r["energy_trace"].any()
        assert r["choice_trace"].shape == (B, 3, N) and r["rotamer"].shape == (B, N) and r["packed"].dtype == torch.bool


# ---- metrics.pack_samples and backbone="packed" --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_pack_samples_after_sample(model):
    B, L, NS = 4, 40, 3
    batch = synth.make_pocket_batch(B, L, 12, seed=71)
    noise = synth.make_noise(B, L, NS, seed=72)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    res_mask = dev_batch["res_mask"].bool()
    gen = dev_batch["generate_mask"].bool() & res_mask
    before = {bb: (metrics.binding_energy(final, dev_batch, backbone=bb), metrics.docking_quality(final, dev_batch, backbone=bb))
              for bb in ("full_atom", "frames")}
    out = metrics.pack_samples(final, dev_batch)
    assert out["pos_heavyatom"].shape == (B, L, 15, 3) and out["pos_heavyatom"].dtype == torch.float32
    assert out["mask_heavyatom"].shape == (B, L, 15) and out["mask_heavyatom"].dtype == torch.bool
    assert out["chi"].shape == (B, L, 4) and out["rotamer"].shape == (B, L) and out["rotamer"].dtype == torch.int32
    assert out["energy_trace"].shape == (B, 9) and out["energy_trace"].dtype == torch.float64 and out["sweeps_run"].shape == (B,)
    for k in ("clash_atoms_before", "clash_atoms_after", "clash_atoms_cross_before", "clash_atoms_cross_after"):
        assert out[k].shape == (B,) and out[k].dtype == torch.int64, k
    for k in ("energy_before", "energy_after", "residue_correct"):
        assert out[k].shape == (B,) and out[k].dtype == torch.float64, k
    assert out["chi_mae"].shape == (B, 4) and out["chi_correct"].shape == (B, 4)
    assert torch.isfinite(out["energy_before"]).all() and torch.isfinite(out["energy_after"]).all()
    assert torch.equal(out["rotamer"] >= 0, gen & (cu(final["seqs"]) < 20))
    rec = (~gen)[:, :, None, None].expand(B, L, 15, 3)
    assert torch.equal(out["pos_heavyatom"][rec], dev_batch["pos_heavyatom"][:, :, :15].float()[rec])
    assert (out["energy_trace"][:, 1:] <= out["energy_trace"][:, :-1] + 1e-3).all()
    assert torch.equal(out["energy_before"], before["frames"][0]["energy"])
    print("pack_samples: energy", [round(v, 2) for v in out["energy_before"].tolist()], "->", [round(v, 2) for v in out["energy_after"].tolist()],
          "clash atoms", out["clash_atoms_before"].tolist(), "->", out["clash_atoms_after"].tolist(),
          "chi1 mae", [round(v, 1) for v in out["chi_mae"][:, 0].tolist()])
    # backbone="packed" is the "frames" complex through pack_sidechains with the defaults
    packed = metrics.binding_energy(final, dev_batch, backbone="packed")
    aa = torch.where(gen, cu(final["seqs"]), cu(final["seqs_1"]))
    again = geometry.interface_energy(out["pos_heavyatom"], out["mask_heavyatom"] & res_mask[:, :, None], aa, gen)
    assert torch.equal(packed["energy"], again["energy"]) and torch.equal(packed["energy"], out["energy_after"])
    for fn in (metrics.docking_quality, metrics.local_accuracy, metrics.structural_violations, metrics.interface_area,
               metrics.secondary_structure, metrics.relax_samples):
        kw = dict(steps=5) if fn is metrics.relax_samples else {}
        assert len(fn(final, dev_batch, backbone="packed", **kw)) > 0, fn.__name__
    # "full_atom" and "frames" are what they were before "packed" was used, bit for bit
    for bb, (e0, d0) in before.items():
        e1, d1 = metrics.binding_energy(final, dev_batch, backbone=bb), metrics.docking_quality(final, dev_batch, backbone=bb)
        for ref, new in ((e0, e1), (d0, d1)):
            for k in ref:
                assert torch.equal(_bits({k: ref[k]})[k], _bits({k: new[k]})[k]), (bb, k)
