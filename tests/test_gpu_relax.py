"""GPU checks of the restrained relaxation: pf_relax_energy_fwd (geometry.relax_energy) against the numpy float64 oracle
(relax_oracle.py) on the tile edges of a 16-residue tile; pf_relax_fwd (geometry.relax) on hand-computed minima, on its own invariants
(a monotone trace, the step rule, bit-identical fixed atoms), against the oracle replaying the device's decisions, for bitwise
repeatability and independence of the batch, for its effect on the clashes that geometry.structural_violations flags, and for peak
memory; metrics.relax_samples after a short sample() run.  The comparison rule is derived in relax_cases.py.  The force field is a
restraint field of this package's own terms: it is not Amber and not Rosetta."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import relax_cases as RC  # noqa: E402
import relax_oracle as RO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import relax as _is_there  # noqa: E402,F401


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def run_energy(case, movable=None, **kw):
    out = geometry.relax_energy(cu(case["pos"]), cu(case["ref_pos"]), cu(case["atom_mask"]), cu(case["aa"]), cu(case["residue_index"]),
                                cu(case["movable"] if movable is None else movable), **kw)
    torch.cuda.synchronize()
    return out


def run_relax(case, steps, pos=None, movable=None, **kw):
    out = geometry.relax(cu(case["pos"] if pos is None else pos), cu(case["atom_mask"]), cu(case["aa"]), cu(case["residue_index"]),
                         cu(case["movable"] if movable is None else movable), steps=steps, **kw)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(out):
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    return {k: (v.view(view[v.dtype]) if v.dtype in view else v) for k, v in out.items()}


# ---- energy and gradient against the float64 oracle --------------------------------------------------------------------------------

SHAPES = {1: 6, 2: 6, 15: 6, 16: 6, 17: 6, 33: 6, 52: 6, 144: 2}
ENERGY_KEYS = {"terms": (torch.float64, (4,)), "energy": (torch.float64, ()), "gradient": (torch.float32, (15, 3)),
               "energy_atom": (torch.float32, (15,)), "terms_atom": (torch.float32, (15, 4))}
STIFF = dict(k_rest=3.0, k_intra=120.0, k_bond=450.0, k_angle=80.0, k_clash=50.0, clash_overlap_tolerance=1.2, clash_margin=0.35)


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_energy_and_gradient_match_oracle(N):
    B = SHAPES[N]
    case = RC.make_case(4200 + N, B, N)
    everything = np.ones((B, N), bool)
    runs = [dict(), dict(movable=everything)]
    if N in (17, 52):
        runs.append(dict(STIFF))
    worst, clash = 0.0, 0.0
    for kw in runs:
        out = run_energy(case, **kw)
        for k, (dt, shape) in ENERGY_KEYS.items():
            assert out[k].dtype == dt and out[k].shape == ((B,) if k in ("terms", "energy") else (B, N)) + shape, k
        got = host(out)
        oracles = RC.oracle(case, **kw)
        worst = max(worst, RC.check(got, case, oracles))
        clash += sum(o["terms"][3] for o in oracles)
        if "movable" not in kw:                             # structure 0 has nothing movable
            assert not got["gradient"][0].any() and got["energy"][0] == 0.0 and not got["terms"][0].any()
        else:
            assert all(o["terms"][0] > 0 and (o["terms"][1] > 0 or N == 1) for o in oracles)
            assert N <= 2 or all(o["terms"][2] > 0 for o in oracles[2:])
    print(f"N = {N}: clash energy {clash:.1f}, largest error / bound = {worst:.4f}")
    assert clash > 0 or N == 1


def test_rigid_shift_changes_nothing_beyond_the_bound():
    """coordinates on a grid of 2^-12 A, so that the shift by (50, -30, 20) is exact in fp32 and the two oracles are the same"""
    case = RC.make_case(4301, 3, 52)
    shift = np.array([50.0, -30.0, 20.0], np.float32)
    for k in ("pos", "ref_pos"):
        case[k] = (np.round(case[k] * 4096.0) / 4096.0).astype(np.float32)
    moved = dict(case, pos=case["pos"] + shift, ref_pos=case["ref_pos"] + shift)
    assert np.array_equal(moved["pos"].astype(np.float64), case["pos"].astype(np.float64) + shift.astype(np.float64))
    o_here, o_there = RC.oracle(case), RC.oracle(moved)
    for a, b in zip(o_here, o_there):
        assert np.abs(a["terms"] - b["terms"]).max() <= 1e-9 * max(1.0, a["energy"])
        assert np.abs(a["gradient"] - b["gradient"]).max() <= 1e-9 * max(1.0, np.abs(a["gradient"]).max())
    RC.check(host(run_energy(case)), case, o_here)
    RC.check(host(run_energy(moved)), moved, o_there)
    assert o_here[1]["terms"][3] > 0


# ---- hand-computed cases -----------------------------------------------------------------------------------------------------------

def test_two_overlapping_atoms_reach_the_closed_form():
    """(a) x - x0 = k_clash (o0 + margin) / (k_rest + k_clash) = 200 * 0.5 / 210 (relax_cases.two_atoms), to 1e-4 A after 200 steps"""
    case, x0, disp = RC.two_atoms()
    out = host(run_relax(case, 200))
    assert abs(float(out["pos"][0, 1, 1, 0]) - x0 - disp) <= 1e-4, (out["pos"][0, 1, 1, 0], x0 + disp)
    moved = out["pos"] != case["pos"]
    assert moved[0, 1, 1, 0] and moved.sum() == 1                               # nothing else changed, bit for bit
    assert abs(out["rmsd"][0] - disp) <= 1e-4 and out["terms_initial"][0, 3] > 0 and not out["terms_initial"][0, :3].any()
    e_min = 0.5 * 10.0 * disp ** 2 + 0.5 * 200.0 * (0.5 - disp) ** 2
    assert abs(out["energy_trace"][0, -1] - e_min) <= 1e-4 * e_min


def test_stretched_bond_reaches_the_closed_form():
    """(b) t = k_bond s / (k_bond + 4 k_rest) along the bond's axis (relax_cases.stretched_bond: why k_rest = 0.01, 1000 steps and
    2e-4 A), the intra term below 1e-6"""
    case, axis, t = RC.stretched_bond()
    out = host(run_relax(case, RC.STRETCH_STEPS, k_rest=RC.STRETCH_K_REST))
    moved = out["pos"][0, 1, :4].astype(np.float64) - case["pos"][0, 1, :4]
    print("stretched bond: largest deviation from the closed form", np.abs(moved + t * axis).max(), "terms", out["terms_final"][0])
    assert np.abs(moved + t * axis).max() <= RC.STRETCH_TOL
    assert out["terms_final"][0, 1] < 1e-6 and out["terms_final"][0, 3] == 0
    assert np.array_equal(out["pos"][0, 0], case["pos"][0, 0])


def test_a_residue_at_its_reference_does_not_move():
    """(c) E = 0, no gradient, the output bit-equal to the input, frozen from the start"""
    case = RC.lone_residue()
    e = host(run_energy(case))
    assert e["energy"][0] == 0.0 and not e["gradient"].any() and not e["terms_atom"].any()
    out = host(run_relax(case, 7))
    assert np.array_equal(out["pos"], case["pos"]) and not out["energy_trace"].any() and not out["accepted"].any()
    assert out["iterations"][0] == 0 and out["grad_max"][0] == 0.0 and out["rmsd"][0] == 0.0
    assert (out["step_size"] == np.float32(0.002)).all()


# ---- properties of relax -----------------------------------------------------------------------------------------------------------

def test_relax_invariants():
    B, N, steps = 4, 33, 30
    case = RC.start_case(4302, N, B)
    case["movable"][0] = False
    pos16 = np.concatenate([case["pos"], np.full((B, N, 1, 3), 7.25, np.float32)], 2)       # a slot beyond the 15
    case16 = dict(case, pos=pos16, ref_pos=pos16, atom_mask=np.concatenate([case["atom_mask"], np.ones((B, N, 1), bool)], 2))
    out = run_relax(case16, steps)
    assert out["pos"].shape == (B, N, 16, 3) and out["pos"].dtype == torch.float32
    for k, dt, shape in (("terms_initial", torch.float64, (B, 4)), ("terms_final", torch.float64, (B, 4)),
                         ("energy_trace", torch.float64, (B, steps + 1)), ("accepted", torch.bool, (B, steps)),
                         ("step_size", torch.float32, (B, steps)), ("grad_max", torch.float32, (B,)), ("iterations", torch.int32, (B,)),
                         ("rmsd", torch.float64, (B,))):
        assert out[k].dtype == dt and out[k].shape == shape, k
    got = host(out)
    trace, acc, alpha = got["energy_trace"], got["accepted"], got["step_size"]
    assert (np.diff(trace, axis=1) <= 0).all() and (np.diff(trace, axis=1)[acc] <= 0).all()
    assert (np.diff(trace, axis=1)[~acc] == 0).all()
    assert (trace[1:, -1] < trace[1:, 0]).all() and acc[1:].any(1).all() and (~acc[1:]).any(1).all()
    # bit for bit: the trace starts at relax_energy of the input and ends at relax_energy of the output
    first = run_energy(case16)
    last = run_energy(dict(case16, pos=got["pos"]))
    assert torch.equal(out["energy_trace"][:, 0], first["energy"]) and torch.equal(out["terms_initial"], first["terms"])
    assert torch.equal(out["terms_final"], last["terms"]) and torch.equal(out["energy_trace"][:, -1], last["energy"])
    assert torch.equal(out["grad_max"], last["gradient"].abs().amax((1, 2, 3)))
    # the step rule, exactly, in fp32
    assert (alpha[:, 0] == np.float32(0.002)).all()
    for b in range(1, B):
        assert got["iterations"][b] == steps
        for i in range(steps - 1):
            assert alpha[b, i + 1] == np.float32(1.2 if acc[b, i] else 0.5) * alpha[b, i], (b, i)
    # structure 0 has nothing movable: frozen at once
    assert got["iterations"][0] == 0 and not acc[0].any() and (trace[0] == 0).all() and (alpha[0] == np.float32(0.002)).all()
    # atoms that do not move and the slot beyond the 15 are the input's bits
    rad = geometry.sasa_radius_table().numpy()
    aa = case["aa"]
    moving = case["atom_mask"] & (rad[np.where((aa < 0) | (aa > 20), 20, aa)] > 0) & case["movable"][:, :, None]
    same = (got["pos"].view(np.int32) == pos16.view(np.int32)).all(-1)
    assert same[:, :, 15].all() and same[:, :, :15][~moving].all() and not same[:, :, :15][moving].all()
    sq = ((got["pos"][:, :, :15].astype(np.float64) - pos16[:, :, :15]) ** 2).sum(-1) * moving
    assert np.allclose(got["rmsd"][1:], np.sqrt(sq.sum((1, 2))[1:] / moving.sum((1, 2))[1:]), rtol=1e-12, atol=0)
    # nothing movable anywhere: the output is the input; steps = 0 is valid
    still = host(run_relax(case16, 5, movable=np.zeros((B, N), bool)))
    assert np.array_equal(still["pos"].view(np.int32), pos16.view(np.int32)) and not still["energy_trace"].any()
    zero = run_relax(case16, 0)
    assert zero["energy_trace"].shape == (B, 1) and zero["accepted"].shape == (B, 0) and zero["step_size"].shape == (B, 0)
    assert torch.equal(zero["energy_trace"][:, 0], first["energy"]) and torch.equal(zero["terms_final"], first["terms"])
    assert np.array_equal(zero["pos"].cpu().numpy().view(np.int32), pos16.view(np.int32))


# ---- the oracle replays the device's decisions -----------------------------------------------------------------------------------

def test_replay():
    """40 iterations from the clashing case of relax_cases.REPLAY_SEED.  Positions: within 4 x the largest deviation between the
    oracle replayed in float32 and in float64 (the factor covers the kernel's other summation order), at least 1e-5 A.  Decisions:
    the sign of the oracle's float64 dE unless |dE| is inside the bound of the comparison, taken at every iteration as the energy
    bound at x plus that at the trial y (relax_cases.decision_bounds: a near decision); near decisions in at most 10 % of the
    iterations."""
    steps = RC.REPLAY_STEPS
    case = RC.start_case()
    got = host(run_relax(case, steps))
    acc = got["accepted"][0]
    args = (case["pos"][0], case["atom_mask"][0], case["aa"][0], case["residue_index"][0], case["movable"][0])
    hi = RO.minimise(*args, steps, replay=acc, **RC.decision_bounds(case))
    lo = RO.minimise(*args, steps, replay=acc, dtype=np.float32)
    tol = max(4 * float(np.abs(hi["pos"] - lo["pos"]).max()), 1e-5)
    dev = float(np.abs(got["pos"][0].astype(np.float64) - hi["pos"]).max())
    bound = hi["decision_bound"]
    near = np.abs(hi["delta_e"]) <= bound
    print(f"replay: tolerance {tol:.3e} A (float32 against float64 oracle {tol / 4:.3e}), device against oracle {dev:.3e} A, "
          f"{int(acc.sum())} of {steps} accepted, {int(near.sum())} near decisions, decision bounds {bound.min():.3f} .. {bound.max():.3f}")
    assert dev <= tol, (dev, tol)
    assert ((hi["delta_e"] <= 0) == acc)[~near].all() and near.mean() <= 0.1
    assert acc.any() and not acc.all()
    assert np.abs(got["energy_trace"][0] - hi["energy_trace"]).max() <= bound.max()
    assert np.array_equal(got["step_size"][0], hi["step_size"])


# ---- repeatability -----------------------------------------------------------------------------------------------------------------

def test_bitwise_repeatable_and_independent_of_batch_and_order():
    B, N, steps = 8, 100, 20
    case = RC.start_case(4311, N, B)
    a, b = _bits(run_relax(case, steps)), _bits(run_relax(case, steps))
    rev = _bits(run_relax({k: v[::-1].copy() for k, v in case.items()}, steps))
    one = _bits(run_relax({k: v[3:4] for k, v in case.items()}, steps))
    assert bool(a["accepted"].any(1).all()) and not bool(a["accepted"].all())
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], rev[k].flip(0)), k
        assert torch.equal(a[k][3], one[k][0]), k
    e = _bits(run_energy(case, movable=np.ones((B, N), bool)))
    e1 = _bits(run_energy({k: v[5:6] for k, v in case.items()}, movable=np.ones((1, N), bool)))
    for k in e:
        assert torch.equal(e[k][5], e1[k][0]), k


# ---- effect --------------------------------------------------------------------------------------------------------------------------

def test_relaxation_removes_clashes():
    """the clashing complex of the replay test, 200 iterations: strictly fewer moving atoms flagged by geometry.structural_violations
    and a strictly lower energy (the counts are in NOTES.md; no ratio is asserted)"""
    case = RC.start_case()
    out = run_relax(case, 200)
    gen = cu(case["movable"])
    flagged = []
    for pos in (cu(case["pos"]), out["pos"]):
        v = geometry.structural_violations(pos, cu(case["atom_mask"]), cu(case["aa"]), cu(case["residue_index"]), query=gen, group=gen)
        flagged.append(int((v["clash_atom"] & gen[:, :, None]).sum()))
    trace = out["energy_trace"][0].cpu().numpy()
    print(f"effect: flagged moving atoms {flagged[0]} -> {flagged[1]}, energy {trace[0]:.1f} -> {trace[-1]:.1f}, "
          f"rmsd {float(out['rmsd'][0]):.3f} A, {int(out['accepted'].sum())} of 200 accepted")
    assert flagged[0] == RC.flagged(case, 0, case["pos"][0]) > 0
    assert flagged[1] < flagged[0] and trace[-1] < trace[0]


# ---- memory, empty batches ---------------------------------------------------------------------------------------------------------

def test_peak_memory_is_not_pair_sized():
    """B = 4, N = 144: one [4, 2160, 2160] fp32 tensor is 74.6 MB; the call may hold a tenth of that beyond its outputs"""
    B, N = 4, 144
    case = RC.start_case(4321, N, B)
    args = [cu(case[k]) for k in ("pos", "atom_mask", "aa", "residue_index", "movable")]
    geometry.relax(*[t[:1] for t in args], steps=1)          # the constant tables are on the device
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = geometry.relax(*args, steps=10)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    assert peak - base <= 0.1 * (B * 2160 * 2160 * 4) + out_bytes, (peak - base, out_bytes)
    assert bool(out["accepted"].any())


def test_empty_batches_launch_nothing():
    for B, N in ((0, 5), (3, 0)):
        pos, mask = torch.zeros(B, N, 15, 3).cuda(), torch.ones(B, N, 15, dtype=torch.bool).cuda()
        aa, idx = torch.zeros(B, N, dtype=torch.int64).cuda(), torch.zeros(B, N, dtype=torch.int32).cuda()
        mov = torch.ones(B, N, dtype=torch.bool).cuda()
        e = geometry.relax_energy(pos, pos, mask, aa, idx, mov)
        assert e["gradient"].shape == (B, N, 15, 3) and e["energy"].shape == (B,) and not e["energy"].any()
        r = geometry.relax(pos, mask, aa, idx, mov, steps=3)
        assert r["pos"].shape == (B, N, 15, 3) and r["energy_trace"].shape == (B, 4) and not r["energy_trace"].any()
        assert r["accepted"].shape == (B, 3) and r["rmsd"].shape == (B,) and r["iterations"].shape == (B,)


# ---- metrics.relax_samples ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_relax_samples_after_sample(model):
    B, L, NS, steps = 4, 40, 3, 60
    batch = synth.make_pocket_batch(B, L, 12, seed=71)
    noise = synth.make_noise(B, L, NS, seed=72)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    res_mask = dev_batch["res_mask"].bool()
    gen = dev_batch["generate_mask"].bool() & res_mask
    for backbone in ("full_atom", "frames"):
        out = metrics.relax_samples(final, dev_batch, backbone=backbone, steps=steps)
        assert out["pos_heavyatom"].shape == (B, L, 15, 3) and out["pos_heavyatom"].dtype == torch.float32
        assert out["mask_heavyatom"].shape == (B, L, 15) and out["mask_heavyatom"].dtype == torch.bool
        for k in ("rmsd_heavy", "relax_energy_before", "relax_energy_after", "energy", "energy_relaxed"):
            assert out[k].shape == (B,) and out[k].dtype == torch.float64 and torch.isfinite(out[k]).all(), k
        for k in ("terms_before", "terms_after"):
            assert out[k].shape == (B, 4) and out[k].dtype == torch.float64 and (out[k] >= 0).all(), k
        for k in ("clash_atoms_before", "clash_atoms_after", "clash_atoms_cross_before", "clash_atoms_cross_after"):
            assert out[k].shape == (B,) and out[k].dtype == torch.int64, k
        for k in ("clashing", "clashing_relaxed"):
            assert out[k].shape == (B,) and out[k].dtype == torch.bool, k
        assert out["energy_trace"].shape == (B, steps + 1) and out["accepted"].shape == (B, steps)
        # the receptor is where the batch has it, bit for bit; the generated residues moved
        rec = (~gen)[:, :, None, None].expand(B, L, 15, 3)
        assert torch.equal(out["pos_heavyatom"][rec], dev_batch["pos_heavyatom"][:, :, :15].float()[rec])
        assert (out["rmsd_heavy"] > 0).all() and (out["relax_energy_after"] <= out["relax_energy_before"]).all()
        ref = metrics.binding_energy(final, dev_batch, backbone=backbone)
        assert torch.equal(out["energy"], ref["energy"]) and torch.equal(out["clashing"], ref["clashing"])
        print(backbone, "clash atoms", out["clash_atoms_before"].tolist(), "->", out["clash_atoms_after"].tolist(),
              "energy", [round(v, 2) for v in out["energy"].tolist()], "->", [round(v, 2) for v in out["energy_relaxed"].tolist()])
        assert (out["clash_atoms_after"] <= out["clash_atoms_before"]).all()
        assert (out["clash_atoms_cross_after"] <= out["clash_atoms_after"]).all()
        again = geometry.interface_energy(out["pos_heavyatom"], out["mask_heavyatom"], torch.where(gen, cu(final["seqs"]), cu(final["seqs_1"])), gen)
        assert torch.equal(out["energy_relaxed"], again["energy"])
