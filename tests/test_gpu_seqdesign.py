"""GPU checks of the fixed-backbone sequence design, pf_sequence_design_fwd (geometry.design_sequence), against the numpy float64 oracle
(seqdesign_oracle.py): the self energies, the start, the first total and the profile on the two sides of the 16-residue environment
tile; a caller's rotamer table on the row-pass and wave edges; 64 and 65 designed residues; the search, replayed visit by visit from
the device's own states; bit-equality with pf_mutation_scan_fwd; the local-minimum certificate; the brute-force minimum of the seeded
small cases; hand-made cases; bitwise repeatability and independence of the batch; peak memory; metrics.design_sequences after a short
sample() run.  The comparison rule is pack_cases.bound (seqdesign_cases.py).  The call is an iterated-conditional-modes search with this
package's own pair energy: it is not ProteinMPNN and not Rosetta fixbb."""
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
import seqdesign_cases as DC  # noqa: E402
import seqdesign_oracle as DO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import design_sequence as _is_there  # noqa: E402,F401
from test_gpu_pack import within  # noqa: E402

KEYS = DC.KEYS


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def run(case, **kw):
    for k in ("candidates", "ref_energy"):
        if kw.get(k) is not None:
            kw[k] = cu(kw[k])
    out = geometry.design_sequence(*[cu(case[k]) for k in KEYS], **kw)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(out):
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    return {k: (v.view(view[v.dtype]) if v.dtype in view else v) for k, v in out.items()}


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def state_of(got, b, o):
    return [(int(got["aa"][b, q]), int(got["rotamer"][b, q])) for q in o.dlist]


def check_structure(case, got, b, o, state, M, chi_tab):
    """the output structure of sample b against the oracle's for `state`; what is not designed comes back bit for bit"""
    A = case["pos"].shape[2]
    aa, pos, mask, chi, rot = o.output(state)
    assert np.array_equal(got["aa"][b], aa) and np.array_equal(got["rotamer"][b], rot), b
    assert np.array_equal(got["atom_mask"][b], mask), b
    if mask.any():
        assert np.abs(got["pos"][b].astype(np.float64) - pos)[mask].max() <= PC.build_err(M), b
    want_chi = np.zeros((o.N, 4), np.float32)
    for p, q in enumerate(o.dlist):
        want_chi[q] = chi_tab[state[p][0], state[p][1]]
    assert np.array_equal(bits32(got["chi"][b]), bits32(want_chi)), b
    un = ~o.designed
    assert np.array_equal(bits32(got["pos"][b][un][:, :A]), bits32(case["pos"][b][un])), b
    assert np.array_equal(got["atom_mask"][b][un][:, :A], case["atom_mask"][b][un]), b
    keep = [0, 1, 2, 3] + ([14] if A > 14 else [])
    assert np.array_equal(bits32(got["pos"][b][:, keep]), bits32(case["pos"][b][:, keep])), b
    assert np.array_equal(got["atom_mask"][b][:, keep], case["atom_mask"][b][:, keep]), b
    assert np.array_equal(got["aa"][b][un], case["aa"][b][un]) and (got["rotamer"][b][un] == -1).all()
    assert np.isposinf(got["profile"][b][un]).all() and (got["profile_rotamer"][b][un] == -1).all()
    assert not got["energy_self_best"][b][un].any() and not got["energy_residue"][b][un].any() and not got["n_candidates"][b][un].any()


def check_start(case, oracles, got, M, chi_tab, profile_of=(0,)):
    """a sweeps=0 run against the oracle: which residues are designed, E_self and the start, the first total, the output structure
    and, for the structures `profile_of`, the profile against the start.  -> the largest |E_self - oracle| / bound"""
    worst = 0.0
    B, N = case["aa"].shape
    assert got["energy_trace"].shape == (B, 1) and got["changed"].shape == (B, 0) and got["changed_types"].shape == (B, 0)
    assert got["profile"].shape == (B, N, 20) and got["designed"].dtype == np.bool_ and not got["sweeps_run"].any()
    for b, o in enumerate(oracles):
        assert np.array_equal(got["designed"][b], o.designed) and got["status"][b] == o.status, b
        state = state_of(got, b, o)
        for p, q in enumerate(o.dlist):
            keys, z = o.flat_self(p)
            assert got["n_candidates"][b, q] == len(o.types[p])
            assert state[p] in keys, (b, q, state[p])
            k, bnd = keys.index(state[p]), DC.bound(z, M)
            err = abs(float(got["energy_self_best"][b, q]) - z["E"][k])
            assert err <= bnd[k], (b, q, state[p], err, bnd[k])
            assert within(z["E"], k, bnd), (b, q, state[p], z["E"][k], z["E"].min())
            worst = max(worst, err / bnd[k]) if bnd[k] > 0 else worst
        tot = o.total(state)
        assert abs(got["energy_trace"][b, 0] - tot["E"]) <= DC.bound(tot, M), (b, got["energy_trace"][b, 0], tot["E"])
        check_structure(case, got, b, o, state, M, chi_tab)
        if b in profile_of:
            check_profile(got, b, o, state, M)
    return worst


def check_profile(got, b, o, state, M):
    """profile[q,t] = min_r conditional(q,t,r) against `state`, by the decision rule per type; +inf / -1 for a non-candidate"""
    for p, q in enumerate(o.dlist):
        for t in range(20):
            r = int(got["profile_rotamer"][b, q, t])
            if t not in o.types[p]:
                assert r == -1 and np.isposinf(got["profile"][b, q, t]), (b, q, t)
                continue
            z = o.conditional(p, t, state)
            bnd = DC.bound(z, M)
            assert 0 <= r < len(z["E"]) and within(z["E"], r, bnd), (b, q, t, r)
            assert abs(float(got["profile"][b, q, t]) - z["E"][r]) <= bnd[r], (b, q, t, r)
            if (t, r) == state[p]:                          # energy_residue: E_self plus half of P + F
                want = 0.5 * (z["E"][r] + o.self_[p][t]["E"][r])
                assert abs(float(got["energy_residue"][b, q]) - want) <= bnd[r], (b, q)


# ---- values and start ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", list(SC.SEEDS))
def test_values_and_start(N):
    """B = 4, the two sides of the 16-residue environment tile; structure 1: every residue designed, 2: none; N = 16: 14 atom slots"""
    case = DC.make_case(N)
    oracles, M = DC.oracle(case, key=N), DC.max_coord(case)        # the cap on near pairs is asserted here, before the device runs
    got = host(run(case, sweeps=0, trace=True))
    assert got["choice_trace"].shape == (DC.B, 0, N, 2)
    if N >= 6:
        assert oracles[1].designed.sum() >= 0.6 * N and not oracles[2].designed.any()
    worst = check_start(case, oracles, got, M, PO.rotamer_table()[0], profile_of=(0,) if N >= 6 else (0, 1, 2, 3))
    print(f"N = {N}: largest |E_self - oracle| / bound = {worst:.3f}")


def test_rotamer_tile_edges():
    """a caller's table: rows one below, at and one above the multiples of the self kernel's 256-row pass, counts 63, 64, 65 around
    a wave of the argmin, counts 1 and 128; random table energies; and reference energies"""
    case, table = SC.edge_case(), SC.edge_table()
    case["designed"] = case.pop("positions")
    case.pop("group")
    ref = np.linspace(-0.4, 0.4, 20).astype(np.float32)
    oracles, M = DC.oracle(case, key="edge", rotamers=table, ref_energy=ref), DC.max_coord(case)
    got = host(run(case, rotamers=tuple(torch.from_numpy(v) for v in table), ref_energy=ref, sweeps=0))
    worst = check_start(case, oracles, got, M, table[0], profile_of=(0, 1))
    assert all(len(o.dlist) == 3 for o in oracles)
    print(f"tile edges: largest |E_self - oracle| / bound = {worst:.3f}")


@pytest.mark.parametrize("n", [64, 65])
def test_64_and_65_designed_residues(n):
    """N = 80: 64 designed residues are designed, 65 are one too many: status 1, and the sample comes back as if nothing were designed;
    the other sample of the batch does not notice"""
    case = DC.many_case(n)
    idx = PO.res_index()
    one = np.zeros(20, bool)
    one[[idx["ALA"], idx["SER"]]] = True
    cand = np.broadcast_to(one, (2, 80, 20))
    oracles, M = DC.oracle(case, candidates=cand), DC.max_coord(case)
    out = run(case, candidates=one, sweeps=0)
    got = host(out)
    assert got["status"].tolist() == [int(n > 64), 0] and got["designed"][0].sum() == (n if n <= 64 else 0) and got["designed"][1].sum() == 4
    check_start(case, oracles, got, M, PO.rotamer_table()[0], profile_of=(1,))
    if n > 64:
        assert not got["energy_trace"][0].any() and (got["rotamer"][0] == -1).all() and np.array_equal(got["aa"][0], case["aa"][0])
        assert np.array_equal(bits32(got["pos"][0]), bits32(case["pos"][0])) and np.array_equal(got["atom_mask"][0], case["atom_mask"][0])
    alone = _bits(run({k: v[1:2] for k, v in case.items()}, candidates=one, sweeps=0))
    for k, v in _bits(out).items():
        assert torch.equal(v[1], alone[k][0]), k


# ---- the search, replayed ------------------------------------------------------------------------------------------------------------

_REPLAYED = {}


def replay_run(N, sweeps):
    if N not in _REPLAYED:
        case = DC.make_case(N, limit=8)
        _REPLAYED[N] = (case, DC.oracle(case, key=("replay", N)), DC.max_coord(case), host(run(case, sweeps=0)),
                        host(run(case, sweeps=sweeps, trace=True)))
    return _REPLAYED[N]


@pytest.mark.parametrize("N,sweeps", [(17, 8), (33, 4)])
def test_replay(N, sweeps):
    case, oracles, M, first, got = replay_run(N, sweeps)
    B = DC.B
    assert got["choice_trace"].shape == (B, sweeps, N, 2) and got["energy_trace"].shape == (B, sweeps + 1)
    assert np.array_equal(got["energy_self_best"], first["energy_self_best"]) and np.array_equal(got["energy_trace"][:, 0], first["energy_trace"][:, 0])
    late = types = 0
    for b, o in enumerate(oracles):
        assert len(o.dlist) <= 8
        cur = state_of(first, b, o)
        trace, run_n = got["energy_trace"][b], int(got["sweeps_run"][b])
        assert 0 < run_n <= sweeps
        for s in range(run_n):
            changed = changed_t = 0
            for p, q in enumerate(o.dlist):
                keys, z = o.flat(p, cur)
                choice = (int(got["choice_trace"][b, s, q, 0]), int(got["choice_trace"][b, s, q, 1]))
                assert choice in keys and within(z["E"], keys.index(choice), DC.bound(z, M)), (b, s, q, choice)
                changed += choice != cur[p]
                changed_t += choice[0] != cur[p][0]
                cur[p] = choice
            assert (got["choice_trace"][b, s][~o.designed] == -1).all()
            assert int(got["changed"][b, s]) == changed and int(got["changed_types"][b, s]) == changed_t, (b, s)
            tot = o.total(cur)
            bnd = DC.bound(tot, M)
            assert abs(trace[s + 1] - tot["E"]) <= bnd, (b, s, trace[s + 1], tot["E"], bnd)
            assert trace[s + 1] <= trace[s] + bnd, (b, s)                   # never rises by more than the bound
            late += s > 0 and changed > 0
            types += changed_t
            assert (changed == 0) == (s == run_n - 1) or s == sweeps - 1
        assert (got["choice_trace"][b, run_n:] == -1).all() and not got["changed"][b, run_n:].any() and not got["changed_types"][b, run_n:].any()
        assert (trace[run_n + 1:] == trace[run_n]).all()
        assert state_of(got, b, o) == cur
        check_structure(case, got, b, o, cur, M, PO.rotamer_table()[0])
        if b == 0:
            check_profile(got, b, o, cur, M)
    assert types > 0
    print(f"N = {N}: changes after the first sweep in {late} (structure, sweep) pairs; {types} type changes")


def test_local_minimum_certificate():
    """on device values alone: where the search stopped by itself, the chosen type is the best of its profile (ties to the smaller
    type) and its profile rotamer is the chosen rotamer"""
    n = 0
    for N, sweeps in ((17, 8), (33, 4)):
        case, oracles, M, first, got = replay_run(N, sweeps)
        for b, o in enumerate(oracles):
            if not got["sweeps_run"][b] < sweeps:
                continue
            for q in o.dlist:
                t, prof = int(got["aa"][b, q]), got["profile"][b, q]
                assert np.isfinite(prof[t]) and t == int(np.argmin(prof)), (N, b, q)       # (argmin: the first of equal values)
                assert got["profile_rotamer"][b, q, t] == got["rotamer"][b, q], (N, b, q)
                n += 1
    assert n > 0


# ---- against pf_mutation_scan_fwd, bitwise -------------------------------------------------------------------------------------------

def test_bitwise_against_mutation_scan():
    """one designed residue, no reference energies, sweeps = 0: profile has the bits of mutation_scan's energy and the same rotamers;
    the chosen type is the argmin under (value, type); with reference energies it is the argmin of energy + ref_energy in fp32"""
    case = SC.make_case(17)
    b = 1
    ok = (case["aa"][b] >= 0) & (case["aa"][b] <= 19) & case["atom_mask"][b][:, :3].all(-1)
    qs = np.flatnonzero(ok)[[0, 6, -1]]
    sel = np.zeros((3, 17), bool)
    sel[np.arange(3), qs] = True
    rep = {k: np.repeat(case[k][b:b + 1], 3, 0) for k in ("pos", "atom_mask", "aa", "residue_index")}
    scan = geometry.mutation_scan(*[cu(rep[k]) for k in ("pos", "atom_mask", "aa", "residue_index")], cu(sel))
    ref = np.random.default_rng(11).uniform(-2.0, 2.0, 20).astype(np.float32)
    rep["designed"] = sel
    plain, with_ref = run(rep, sweeps=0), run(rep, sweeps=0, ref_energy=ref)
    for i, q in enumerate(qs):
        e, rot = scan["energy"][i, q], scan["rotamer"][i, q]
        assert torch.isfinite(e).all()
        assert torch.equal(plain["profile"][i, q].view(torch.int32), e.view(torch.int32)), q
        assert torch.equal(plain["profile_rotamer"][i, q], rot), q
        t = int(torch.argmin(e))                            # (the first of equal values: the smaller type)
        assert int(plain["aa"][i, q]) == t and int(plain["rotamer"][i, q]) == int(rot[t])
        assert plain["energy_self_best"][i, q] == e[t] and plain["energy_residue"][i, q] == e[t]
        shifted = e + cu(ref)
        t = int(torch.argmin(shifted))
        assert int(with_ref["aa"][i, q]) == t and int(with_ref["rotamer"][i, q]) == int(rot[t])
        assert torch.equal(with_ref["profile"][i, q].view(torch.int32), shifted.view(torch.int32)), q


# ---- the brute-force minimum of the small cases ----------------------------------------------------------------------------------------

def test_small_seeds_reach_the_brute_force_minimum():
    seeds = DC.small_seeds()
    cases = [DC.small_case(s) for s in seeds]
    batch = {k: np.concatenate([c[k] for c, _ in cases]) for k in KEYS}
    cand = np.concatenate([c for _, c in cases])
    got = host(run(batch, candidates=cand, rotamers=tuple(torch.from_numpy(v) for v in DC.small_table()), trace=True))
    clear = 0
    for b, s in enumerate(seeds):
        rep = DC.small_report(s)
        o, M = DC.small_design(s)
        assert abs(got["energy_trace"][b, -1] - rep["best"]) <= DC.bound(o.total(rep["state"]), M), s
        if rep["clear"]:                                    # every runner-up ten bounds away: the device walks the oracle's own path
            clear += 1
            assert state_of(got, b, o) == rep["state"], s
            n = rep["run"]["sweeps_run"]
            assert int(got["sweeps_run"][b]) == n and got["changed"][b, :n].tolist() == rep["run"]["changed"], s
            assert got["changed_types"][b, :n].tolist() == rep["run"]["changed_types"], s
    assert clear >= DC.SMALL_CLEAR


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------

def test_hand_lone():
    """a lone residue: the chosen type is the argmin of its own per-type self energies"""
    case = DC.hand_lone("MET")
    o = DO.Design(*[case[k][0] for k in KEYS])
    keys, z = o.flat_self(0)
    want = keys[int(np.argmin(z["E"]))]
    got = host(run(case))
    assert state_of(got, 0, o) == [want] and int(got["sweeps_run"][0]) == 1 and not got["changed"].any()
    per_type = got["profile"][0, 0]
    assert int(np.argmin(per_type)) == want[0] and got["energy_self_best"][0, 0] == per_type[want[0]]
    assert got["energy_residue"][0, 0] == got["energy_self_best"][0, 0] and (got["energy_trace"][0] == got["energy_trace"][0, 0]).all()
    assert np.array_equal(got["pos"][0, 0, :4], case["pos"][0, 0, :4])


def test_hand_pocket():
    """the pocket of lone carbons where a LEU's CD1 and CD2 would sit: the designed residue becomes hydrophobic and gains more than
    0.5 over ALA; with ref_energy[LEU] = +10 it is no longer LEU"""
    idx = PO.res_index()
    case = DC.hand_pocket()
    got = host(run(case))
    t = int(got["aa"][0, 0])
    hydrophobic = {idx[n] for n in ("LEU", "ILE", "VAL", "MET", "PHE", "TRP", "TYR")}
    assert got["designed"][0].tolist() == [True] + [False] * (case["aa"].shape[1] - 1)
    assert t in hydrophobic, t
    assert got["profile"][0, 0, t] - got["profile"][0, 0, idx["ALA"]] < -0.5
    assert got["profile"][0, 0, idx["LEU"]] - got["profile"][0, 0, idx["ALA"]] < -0.5
    leu_only = np.zeros(20, bool)
    leu_only[[idx["LEU"], idx["ALA"]]] = True
    assert int(host(run(case, candidates=leu_only))["aa"][0, 0]) == idx["LEU"]
    ref = np.zeros(20, np.float32)
    ref[idx["LEU"]] = 10.0
    assert int(host(run(case, candidates=leu_only, ref_energy=ref))["aa"][0, 0]) == idx["ALA"]
    assert int(host(run(case, ref_energy=ref))["aa"][0, 0]) != idx["LEU"]


def test_hand_pair():
    """two facing designed residues: taking the partner's side chain into account changes the choice that mutation_scan, which can
    only ask about each residue with the other as given, makes.  Asserted on the oracle (test_seqdesign_cpu.py), then on the device."""
    case, cand = DC.hand_pair()
    o = DO.Design(*[case[k][0] for k in KEYS], candidates=cand[0])
    want = o.icm(8)
    scan = geometry.mutation_scan(*[cu(case[k]) for k in KEYS], candidates=cu(cand))
    e, rot = scan["energy"][0].cpu().numpy(), scan["rotamer"][0].cpu().numpy()
    alone = [(int(np.argmin(e[q])), int(rot[q, int(np.argmin(e[q]))])) for q in range(2)]
    got = host(run(case, candidates=cand, trace=True))
    state = state_of(got, 0, o)
    assert state == want["state"] and state != alone
    assert state[0][0] != alone[0][0] and got["changed_types"][0, 0] > 0           # the joint answer differs in type
    assert int(got["sweeps_run"][0]) == want["sweeps_run"] and got["changed"][0, :want["sweeps_run"]].tolist() == want["changed"]
    M = DC.max_coord(case)
    assert o.total(alone)["E"] - got["energy_trace"][0, -1] > 1.0
    assert abs(got["energy_trace"][0, -1] - o.total(state)["E"]) <= DC.bound(o.total(state), M)
    assert got["energy_trace"][0, 0] - got["energy_trace"][0, -1] > 1.0


# ---- repeatability -----------------------------------------------------------------------------------------------------------------

def test_bitwise_repeatable_and_independent_of_batch_and_order():
    case = DC.make_case(17)
    kw = dict(sweeps=3, trace=True, ref_energy=np.linspace(0.3, -0.3, 20))
    a, b = _bits(run(case, **kw)), _bits(run(case, **kw))
    perm = [2, 0, 3, 1]
    shuffled = _bits(run({k: v[perm].copy() for k, v in case.items()}, **kw))
    assert bool(a["changed"].any()) and len(a) == 17
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][perm], shuffled[k]), k
    for i in range(DC.B):
        one = _bits(run({k: v[i:i + 1] for k, v in case.items()}, **kw))
        for k in a:
            assert torch.equal(a[k][i], one[k][0]), (i, k)


# ---- memory, empty batches ---------------------------------------------------------------------------------------------------------

def test_peak_memory_is_the_workspace():
    """B = 4, N = 33: beyond its inputs the call holds its outputs and its workspace, pf_sequence_design_work_bytes(B, N, 108, 64) = B
    (16 + 276 N + 64 (84 + 80 x 108)) bytes: nothing per residue and rotamer atom (the packer's workspace holds 148 bytes per residue
    and rotamer).  Slack: 64 KiB for the allocator's rounding of each of the 17 tensors to 512 bytes and the 80 bytes of ref_energy."""
    case = DC.make_case(33)
    B, N = DC.B, 33
    args = [cu(case["pos"]), cu(case["atom_mask"]).view(torch.uint8), cu(case["aa"]), cu(case["residue_index"]),
            cu(case["designed"]).view(torch.uint8)]
    geometry.design_sequence(*[t[:1] for t in args], sweeps=1)          # the constant tables are on the device
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = geometry.design_sequence(*args, sweeps=2, trace=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    work = _capi.load().pf_sequence_design_work_bytes(B, N, 108, 64)
    assert work == B * (16 + 276 * N + 64 * (84 + 80 * 108))
    assert peak - base <= work + out_bytes + 64 * 1024, (peak - base, work, out_bytes)


def test_empty_batches_launch_nothing():
    for B, N in ((0, 5), (3, 0)):
        pos, mask = torch.zeros(B, N, 15, 3).cuda(), torch.ones(B, N, 15, dtype=torch.bool).cuda()
        aa, idx = torch.zeros(B, N, dtype=torch.int64).cuda(), torch.zeros(B, N, dtype=torch.int32).cuda()
        sel = torch.ones(B, N, dtype=torch.bool).cuda()
        calls = _capi.CALLS
        r = geometry.design_sequence(pos, mask, aa, idx, sel, sweeps=3, trace=True)
        assert _capi.CALLS == calls
        assert r["pos"].shape == (B, N, 15, 3) and r["energy_trace"].shape == (B, 4) and not r["energy_trace"].any()
        assert r["choice_trace"].shape == (B, 3, N, 2) and r["rotamer"].shape == (B, N) and r["designed"].dtype == torch.bool
        assert r["aa"].shape == (B, N) and r["aa"].dtype == torch.int64 and r["profile"].shape == (B, N, 20) and r["status"].shape == (B,)
        assert r["changed_types"].shape == (B, 3) and r["profile_rotamer"].dtype == torch.int32


# ---- metrics.design_sequences --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_design_sequences_after_sample(model):
    B, L, NS = 4, 40, 3
    batch = synth.make_pocket_batch(B, L, 12, seed=71)
    noise = synth.make_noise(B, L, NS, seed=72)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    res_mask = dev_batch["res_mask"].bool()
    gen = dev_batch["generate_mask"].bool() & res_mask
    model_seq, native = cu(final["seqs"]), cu(final["seqs_1"])
    out = metrics.design_sequences(final, dev_batch)
    assert out["seqs"].shape == (B, L) and out["seqs"].dtype == torch.int64
    assert out["pos_heavyatom"].shape == (B, L, 15, 3) and out["pos_heavyatom"].dtype == torch.float32
    assert out["mask_heavyatom"].shape == (B, L, 15) and out["mask_heavyatom"].dtype == torch.bool
    assert out["chi"].shape == (B, L, 4) and out["rotamer"].shape == (B, L) and out["rotamer"].dtype == torch.int32
    assert out["energy_trace"].shape == (B, 9) and out["energy_trace"].dtype == torch.float64 and out["sweeps_run"].shape == (B,)
    assert out["profile"].shape == (B, L, 20) and out["profile"].dtype == torch.float32
    assert out["status"].shape == (B,) and out["status"].dtype == torch.int32 and not out["status"].any()
    for k in ("recovery_native", "recovery_model", "energy_before", "energy_after"):
        assert out[k].shape == (B,) and out[k].dtype == torch.float64, k
    for k in ("changed_from_model", "clash_atoms_cross_before", "clash_atoms_cross_after"):
        assert out[k].shape == (B,) and out[k].dtype == torch.int64, k
    assert torch.isfinite(out["energy_before"]).all() and torch.isfinite(out["energy_after"]).all()
    # designed = the generated residues of a type in 0..19; everything else bit-identical to the rebuilt complex
    designed = out["rotamer"] >= 0
    assert torch.equal(designed, gen & (model_seq < 20)) and bool(designed.any())
    rec = (~gen)[:, :, None, None].expand(B, L, 15, 3)
    assert torch.equal(out["pos_heavyatom"][rec], dev_batch["pos_heavyatom"][:, :, :15].float()[rec])
    start = torch.where(gen, model_seq, native)
    assert torch.equal(out["seqs"][~designed], start[~designed])
    assert (out["energy_trace"][:, 1:] <= out["energy_trace"][:, :-1] + 1e-3).all()
    n = designed.sum(1).double()
    for k, ref in (("recovery_native", native), ("recovery_model", model_seq)):
        again = (designed & (out["seqs"] == ref)).sum(1).double() / n
        assert torch.equal(out[k], again) and bool(((out[k] >= 0) & (out[k] <= 1)).all()), k
    assert torch.equal(out["changed_from_model"], (designed & (out["seqs"] != model_seq)).sum(1))
    before = metrics.binding_energy(final, dev_batch, backbone="frames")
    assert torch.equal(out["energy_before"], before["energy"])
    again = geometry.interface_energy(out["pos_heavyatom"], out["mask_heavyatom"], out["seqs"], gen)
    assert torch.equal(out["energy_after"], again["energy"])
    print("design_sequences: recovery", [round(v, 2) for v in out["recovery_native"].tolist()], "energy",
          [round(v, 2) for v in out["energy_before"].tolist()], "->", [round(v, 2) for v in out["energy_after"].tolist()],
          "sweeps", out["sweeps_run"].tolist())
    # candidates="ALA": every designed residue is ALA (the set holds nothing else), the rest keeps its type
    from pepflowww_amd.preprocess import residue_type
    ala = metrics.design_sequences(final, dev_batch, candidates="ALA", sweeps=2)
    assert bool((ala["seqs"][designed] == residue_type("ALA")).all()) and torch.equal(ala["seqs"][~designed], start[~designed])
    assert torch.equal(ala["recovery_native"], (designed & (native == residue_type("ALA"))).sum(1).double() / n)
