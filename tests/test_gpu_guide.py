"""Guided sampling on a real MI355X: pf_guidance_fwd alone (geometry.ca_potential and the sampler mode through the C ABI), in front of
pf_sampler_step_cond on fabricated "network outputs", and end to end through FlowModel.sample(guide=...).

Tolerances.  Kernel against the float64 oracle (energies, gradient, guided translations, largest shift): 2 fp32 ulp of the tensor's
largest magnitude -- derived, not measured: both sides carry double from the same fp32 inputs and round once; another summation order
in double is ~1e-13 relative.  Behind the step kernel and end to end: the rules of tests/test_gpu_cond.py and
tests/test_gpu_bigshape._compare_traj, unchanged.  The per-step energies of an end-to-end run see predictions that agree with the
oracle's only to the bound _compare_traj holds the trajectory to (dx = 3e-4 of the largest translation): they are held to the first-
order image of that bound, 2 * dx * sum_i |dE_k / dx_i|_1 over the movable rows (the oracle's own autograd gradient, factor 2 for the
second order) + 2 fp32 ulp.  The conditions the cases must meet (every term positive, clip active and inactive, no coincident pair) are
asserted on the CPU in tests/test_guide_cpu.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, geometry, sampler, synth  # noqa: E402
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import guide_cases as GC  # noqa: E402
import guide_oracle as GO  # noqa: E402
import gpu_util as G  # noqa: E402
from cond_oracle import O  # noqa: E402
from test_gpu_bigshape import REL, _compare_traj  # noqa: E402
from test_gpu_cond import STATE, TRAJ, Abi, _check_state, _f64_rule, _wrapped, cu  # noqa: E402

SENTINEL = -7.0


def _two_ulp(got, ref64, what, worst=None):
    """|kernel - float64 oracle| <= 2 fp32 ulp of the tensor's largest magnitude"""
    got, ref64 = got.detach().cpu().double(), ref64.double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), what
    tol = 2.0 * float(np.spacing(np.float32(float(ref64.abs().max()))))
    d = float((got - ref64).abs().max())
    print(f"{what}: |kernel - oracle64| = {d:.3e}, 2 ulp = {tol:.3e}")
    if worst is not None:
        worst.append((d / tol if tol else 0.0, what))
    assert d <= tol, (what, d, tol)


def _classes(case, guide):
    return GO.row_classes(case["batch"]["generate_mask"], case["batch"]["res_mask"], case["flags"][0], GO.params(guide)["hotspots"])


def _params_of(guide):
    return {k: v for k, v in guide.items() if k not in ("hotspots", "restraints")}


# ==== 1: the stand-alone surface ========================================================================================================
@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", ["full", "null_plane"])
def test_ca_potential_vs_float64_oracle(shape, name):
    case, guide = GC.abi_case(shape), GC.abi_guide(shape, name)
    cls = _classes(case, guide)
    grid = CO.make_grid(case["NS"])
    for step in (0, case["NS"] - 1):
        x = torch.where(cls["M"][..., None], case["preds"][step][1], case["gt"][1])
        t = float(grid[step])
        ref_x, ref_e, ref_g, ref_n = GO.guided(x, x, cls, guide, t)
        out = geometry.ca_potential(cu(x), cls["P"], cls["M"], cls["C"], guide.get("hotspots"), guide.get("restraints"), t=t, **_params_of(guide))
        assert out["energy"].shape == (case["B"], 5) and out["grad"].shape == x.shape and out["energy"].is_cuda
        what = f"{shape} {name} step {step}"
        _two_ulp(out["energy"], ref_e, what + " energy")
        _two_ulp(out["grad"], ref_g, what + " gradient")
        _two_ulp(out["guided"], ref_x, what + " guided")
        _two_ulp(out["shift_max"], ref_n.max(1).values, what + " shift_max")
        assert float(out["grad"].cpu()[~cls["M"]].abs().max()) == 0
        assert torch.equal(out["guided"].cpu()[~cls["M"]], x[~cls["M"]])
        again = geometry.ca_potential(cu(x), cls["P"], cls["M"], cls["C"], guide.get("hotspots"), guide.get("restraints"), t=t, **_params_of(guide))
        for k in out:                                          # determinism: the same bits
            assert torch.equal(out[k], again[k]), (what, k)
    assert float(ref_g.abs().max()) > 1


def test_ca_potential_checks_its_arguments():
    case, guide = GC.abi_case("3x16"), GC.abi_guide("3x16", "full")
    cls = _classes(case, guide)
    x = cu(case["gt"][1])
    with pytest.raises(ValueError, match="subset"):
        geometry.ca_potential(x, cls["P"], cls["P"] | cls["C"], cls["C"])
    with pytest.raises(ValueError, match="disjoint"):
        geometry.ca_potential(x, cls["P"], cls["M"], cls["C"] | cls["P"])
    with pytest.raises(ValueError, match="index 16"):
        geometry.ca_potential(x, cls["P"], cls["M"], cls["C"], restraints=[(0, 16, 1.0, 2.0, 1.0)])
    with pytest.raises(_capi.PepflowHipError):
        geometry.ca_potential(case["gt"][1], cls["P"], cls["M"], cls["C"])         # a CPU tensor: no fallback
    zero = geometry.ca_potential(x, cls["P"], cls["M"], cls["C"])                  # all weights zero, no restraints
    assert float(zero["energy"].abs().max()) == 0 and float(zero["grad"].abs().max()) == 0 and torch.equal(zero["guided"], x)


# ==== 2: the sampler mode through the C ABI =============================================================================================
class Guidance:
    """device buffers of one ABI case behind a pf_guidance_args in sampler mode"""

    def __init__(self, case, guide, pred_step=1):
        B, L, NS = case["B"], case["L"], case["NS"]
        rows = B * L
        self.case, self.B, self.L, self.NS = case, B, L, NS
        gen, resm = case["batch"]["generate_mask"], case["batch"]["res_mask"]
        self.packed = sampler.make_guide(guide, B, L, gen, resm)
        plane = sampler.pack_res_flags(*case["flags"], B, L)[1]
        f = lambda *s: torch.full(s, SENTINEL, device=G.dev())  # noqa: E731
        self.t = {"pred_trans": cu(case["preds"][pred_step][1].reshape(rows, 3)), "trans1": cu(case["gt"][1].reshape(rows, 3)),
                  "gen_mask": cu(gen.reshape(rows).float()), "res_mask": cu(resm.reshape(rows).float()), "res_flags": cu(plane.reshape(rows)),
                  "pair_idx": cu(self.packed["pair_idx"]), "pair_par": cu(self.packed["pair_par"]), "params": cu(self.packed["params"]),
                  "ts": cu(CO.make_grid(NS)), "step": torch.zeros(2, dtype=torch.int32, device=G.dev()),
                  "guided_trans": f(rows, 3), "energy": f(NS, B, 5), "shift_max": f(NS, B), "error": torch.zeros(B, dtype=torch.int32, device=G.dev())}
        if self.packed["hotspots"] is not None:
            self.t["hotspots"] = cu(self.packed["hotspots"].reshape(rows))
        a = self.args = _capi.GuidanceArgs()
        for k, v in self.t.items():
            setattr(a, k, v.data_ptr())
        a.B, a.L, a.num_steps, a.sample_bb = B, L, NS, 0          # (the plane is in charge: the scalar says the opposite)

    def run(self, step):
        for k in ("guided_trans", "energy", "shift_max"):
            self.t[k].fill_(SENTINEL)
        self.t["step"][0] = step
        _capi.check(_capi.load().pf_guidance_fwd(C.byref(self.args), _capi.stream_ptr()), "pf_guidance_fwd")
        return {k: self.t[k].cpu().clone() for k in ("guided_trans", "energy", "shift_max", "error")}


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", ["full", "null_plane"])
def test_sampler_mode_vs_oracle_slots_and_untouched_rows(shape, name):
    case, guide = GC.abi_case(shape), GC.abi_guide(shape, name)
    B, L, NS = case["B"], case["L"], case["NS"]
    cls = _classes(case, guide)
    grid = CO.make_grid(NS)
    h = Guidance(case, guide, pred_step=1)
    x_p = case["preds"][1][1]
    for step in (1, NS - 1):
        got = h.run(step)
        ref_x, ref_e, _, ref_n = GO.guided(x_p, case["gt"][1], cls, guide, grid[step])
        what = f"{shape} {name} slot {step}"
        gx = got["guided_trans"].view(B, L, 3)
        _two_ulp(gx, ref_x, what + " guided_trans")
        _two_ulp(got["energy"][step], ref_e, what + " energy")
        _two_ulp(got["shift_max"][step], ref_n.max(1).values, what + " shift_max")
        assert torch.equal(gx[~cls["M"]], x_p[~cls["M"]]), "rows that do not move keep the prediction's bits"
        assert not torch.equal(gx[cls["M"]], x_p[cls["M"]])
        others = [s for s in range(NS) if s != step]
        assert (got["energy"][others] == SENTINEL).all() and (got["shift_max"][others] == SENTINEL).all(), "only slot *step is written"
        assert (got["error"] == 0).all()
        again = h.run(step)
        for k in got:
            assert torch.equal(got[k], again[k]), (what, k, "two runs, the same bits")
    late = h.run(NS)                                           # *step >= num_steps: returns without writing
    assert all((late[k] == SENTINEL).all() for k in ("guided_trans", "energy", "shift_max"))


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_zero_gradient_leaves_the_predictions_bits(shape):
    case, full = GC.abi_case(shape), GC.abi_guide(shape, "full")
    x_p = case["preds"][1][1].reshape(-1, 3)
    zero = {**full, "weights": [0.0] * 4, "restraints": [[(i, j, lo, hi, 0.0) for (i, j, lo, hi, w) in rs] for rs in full["restraints"]]}
    got = Guidance(case, zero).run(1)
    assert torch.equal(got["guided_trans"], x_p) and float(got["energy"][1].abs().max()) == 0 and float(got["shift_max"][1].abs().max()) == 0
    off = Guidance(case, {**full, "t_on": 0.9}).run(0)         # t = 0.01 < t_on: lambda = 0, the energies are still recorded
    assert torch.equal(off["guided_trans"], x_p) and float(off["shift_max"][0].abs().max()) == 0 and float(off["energy"][0].max()) > 0
    on = Guidance(case, {**full, "t_on": 0.9}).run(case["NS"] - 1)
    assert not torch.equal(on["guided_trans"], x_p)


def test_a_restraint_index_outside_the_sample_is_refused_by_the_kernel():
    """the list lives in device memory, so the host entry cannot see it: the kernel skips the pair (it never reads outside the sample's
    rows) and raises the sample's error flag; every output equals the run without that pair"""
    case, guide = GC.abi_case("3x16"), GC.abi_guide("3x16", "full")
    h = Guidance(case, guide)
    slot = len(guide["restraints"][2])
    clean = h.run(1)
    idx, par = h.packed["pair_idx"].clone(), h.packed["pair_par"].clone()
    idx[2, slot], par[2, slot] = torch.tensor([3, case["L"]], dtype=torch.int32), torch.tensor([1.0, 2.0, 1.0])
    idx[3, 0], par[3, 0] = torch.tensor([-1, 2], dtype=torch.int32), torch.tensor([1.0, 2.0, 1.0])
    h.t["pair_idx"].copy_(idx)
    h.t["pair_par"].copy_(par)
    got = h.run(1)
    assert got["error"].tolist() == [0, 0, -1, -1, 0]
    for k in ("guided_trans", "energy", "shift_max"):
        assert torch.equal(got[k], clean[k]), k


# ==== 3: guidance in front of the step kernel ===========================================================================================
@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", ["full", "null_plane"])
def test_guidance_then_step_kernel_vs_oracle(shape, name):
    """pf_guidance_fwd writes the buffer pf_sampler_step_cond reads its translation prediction from; trajectory and the state after
    every Euler step against cond_oracle.sample(preds = the oracle's guided predictions), by the rules of tests/test_gpu_cond.py"""
    case, guide = GC.abi_case(shape), GC.abi_guide(shape, name)
    B, L, NS = case["B"], case["L"], case["NS"]
    rows = B * L
    grid = CO.make_grid(NS)
    s32, s64 = [], []
    o = dict(encoded=case["encoded"], flags=case["flags"])
    ref = CO.sample(None, case["batch"], case["noise"], NS, preds=GO.guided_preds(case, guide, case["flags"], grid, torch.float32), states=s32, **o)
    ref64 = CO.sample(None, case["batch"], case["noise"], NS, preds=GO.guided_preds(case, guide, case["flags"], grid, torch.float64), states=s64,
                      dtype=torch.float64, **o)
    h = Abi(case, case["noise"], grid)
    cond = h.cond(flags=case["flags"])
    gd = Guidance(case, guide)
    raw = torch.zeros(rows, 3, device=G.dev())
    ga = gd.args
    ga.pred_trans, ga.guided_trans = raw.data_ptr(), h.t["pred_trans"].data_ptr()
    ga.res_flags, ga.step, ga.ts = cond.res_flags, h.t["step"].data_ptr(), h.t["ts"].data_ptr()
    gd.t["energy"].fill_(SENTINEL)
    lib, st, nz = _capi.load(), _capi.stream_ptr(), h.noise
    _capi.check(lib.pf_sampler_init_cond(C.byref(h.args), C.byref(cond), nz["rot0"].data_ptr(), nz["trans0"].data_ptr(), nz["ang0"].data_ptr(),
                                         nz["simplex0"].data_ptr(), st), "pf_sampler_init_cond")
    states = []
    for s in range(NS):
        for buf, v in zip((h.t["pred_rot"], raw, h.t["pred_ang_raw"], h.t["pred_logits"]), case["preds"][s]):
            buf.copy_(v.reshape(buf.shape))                    # (the network's translation goes to `raw`: the step kernel reads the guided copy)
        _capi.check(lib.pf_guidance_fwd(C.byref(ga), st), "pf_guidance_fwd")
        _capi.check(lib.pf_sampler_step_cond(C.byref(h.args), C.byref(cond), st), "pf_sampler_step_cond")
        states.append({k: h.t[k].cpu().clone() for k in STATE})
    assert h.t["step"].tolist() == [NS, 0] and (gd.t["energy"] != SENTINEL).all()
    tr = {k: h.t[k].cpu() for k in TRAJ}
    ratios = []
    for i in range(NS):
        assert torch.equal(tr["traj_seq"][i].view(B, L), ref[i]["seqs"]), f"step {i}: flipped draws"
        assert torch.equal(tr["traj_simplex"][i].view(B, L, 20), ref[i]["seqs_simplex"])
        assert torch.equal(tr["traj_rot"][i].view(B, L, 3, 3), ref[i]["rotmats"])
        _f64_rule(tr["traj_trans"][i].view(B, L, 3), ref[i]["trans"], ref64[i]["trans"], f"step {i} traj_trans", ratios)
        assert _wrapped(tr["traj_ang"][i].view(B, L, 5), ref[i]["angles"]) < 5e-6, f"step {i} angles"
    ok = torch.ones(B, L, dtype=torch.bool)
    for s in range(NS - 1):
        ok = ok & s32[s][5]
        _check_state(states[s], s32[s], s64[s], ok, f"{name} state {s}", ratios, L)
    unguided = CO.sample(None, case["batch"], case["noise"], NS, preds=case["preds"], **o)
    assert not torch.equal(unguided[1]["trans"], ref[1]["trans"]), "the guidance must move the trajectory"
    print(f"{shape} {name}: worst kernel deviation / tolerance = {max(ratios)[0]:.3f} ({max(ratios)[1]})")


# ==== 5: FlowModel.sample ===============================================================================================================
@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd, strict=True)
    return m.to(G.dev()).eval()


def _dev(batch):
    return {k: cu(v) for k, v in batch.items()}


def _same_traj(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert torch.equal(x[k], y[k]), (what, i, k)


def _oracle_run(sd, batch, guide, seed):
    """-> (noise with draws widened on the oracle's own guided run, its trajectory, per-step energies [NS, B, 5] float64, the
    positions they were taken at per step)"""
    B, L = batch["aa"].shape
    NS = CC.NS_E2E
    noise = synth.make_noise(B, L, NS, seed=seed)
    with torch.no_grad():
        enc = O.encode(sd, batch)
        grec = []

        def run(rec):
            grec.clear()
            return GO.sample(sd, batch, noise, NS, encoded=enc, guide=guide, rec=rec, grec=grec)
        _, ref = CO.widen_draws(run, noise, batch["generate_mask"])
    return noise, ref, torch.stack([e for e, _, _ in grec]), [x for _, _, x in grec]


def _energy_tolerance(batch, guide, energy, xs):
    """2 * dx * sum over the movable rows of |dE_k / dx_i|_1 at the oracle's own unguided predictions xs + 2 fp32 ulp (module docstring)"""
    gen, resm = batch["generate_mask"].bool(), batch["res_mask"].bool()
    cls = GO.row_classes(gen, resm, True, GO.params(guide)["hotspots"])
    tol = torch.zeros_like(energy)
    for i, x_u in enumerate(xs):
        dx = 3 * REL * float(x_u.abs().max())
        with torch.enable_grad():
            x = x_u.double().requires_grad_(True)
            e = GO.energies(x, cls, guide)
            for k in range(5):
                (g,) = torch.autograd.grad(e[:, k].sum(), x, retain_graph=True)
                tol[i, :, k] = 2 * dx * (g.abs() * cls["M"][..., None]).sum((1, 2))
    return tol + 2.0 * float(np.spacing(np.float32(float(energy.abs().max()))))


@pytest.mark.parametrize("shape", list(CC.E2E_SHAPES))
def test_guided_sample_vs_oracle_replay_second_guide_and_no_leak(model, seeded_sd, shape):
    NS = CC.NS_E2E
    batch = CC.e2e_batch(shape)
    B, L = batch["aa"].shape
    db = _dev(batch)
    plain_noise = synth.make_noise(B, L, NS, seed=5)
    before = model.sample(db, num_steps=NS, noise=plain_noise)
    assert model.last_guidance is None
    for which, seed in (("a", 41), ("b", 42)):                 # 'b' runs on the sampler 'a' built: other weights, hot spots, restraints
        guide = GC.e2e_guide(shape, which)
        noise, ref, energy, xs = _oracle_run(seeded_sd, batch, guide, seed)
        traj = model.sample(db, num_steps=NS, noise=noise, guide=guide)
        rec = model.last_guidance
        _compare_traj(traj, ref, 0, B, NS, f"{shape} guide {which}")
        assert rec["terms"] == GO.TERMS and rec["energy"].shape == (NS, B, 5) and rec["shift_max"].shape == (NS, B) and not rec["energy"].is_cuda
        tol = _energy_tolerance(batch, guide, energy, xs)
        d = (rec["energy"].double() - energy).abs()
        print(f"{shape} guide {which}: worst energy deviation / tolerance = {float((d / tol).max()):.3f}; energies {energy.sum(1)[0].tolist()}")
        assert (d <= tol).all(), (which, float((d / tol).max()))
        assert float(rec["shift_max"].max()) > 0 and float(rec["shift_max"].max()) <= GO.params(guide)["max_shift"] * (1 + 1e-6)
        unguided = model.sample(db, num_steps=NS, noise=noise)
        gen = batch["generate_mask"]
        assert not torch.equal(unguided[1]["trans"][gen], traj[1]["trans"][gen]), "the guidance must change the run"
        eager = model.sample(db, num_steps=NS, noise=noise, guide=guide, use_graph=False)
        _same_traj(traj, eager, f"guide {which}: graph replay vs eager")
        assert torch.equal(model.last_guidance["energy"], rec["energy"]) and torch.equal(model.last_guidance["shift_max"], rec["shift_max"])
    _same_traj(before, model.sample(db, num_steps=NS, noise=plain_noise), "default call after guided calls")
    assert model.last_guidance is None


def test_guide_combines_with_the_conditioned_call(model):
    """a partial start, per-residue switches and allowed classes together with a guide: graph equals eager, rows whose backbone switch
    is off keep the context's translation, and the guide changes the run"""
    NS = CC.NS_E2E
    batch = CC.e2e_batch("L24")
    B, L = batch["aa"].shape
    db = _dev(batch)
    g = torch.Generator().manual_seed(3)
    kw = CC.sample_kwargs({"flags": CC._mixed_flags(B, L, g), "aa_allowed": CC._allowed("random", B, L, g), "t_start": 0.4, "start": "native"})
    noise = synth.make_noise(B, L, NS, seed=12)
    guide = GC.e2e_guide("L24", "a")
    a = model.sample(db, num_steps=NS, noise=noise, guide=guide, **kw)
    rec = model.last_guidance
    _same_traj(a, model.sample(db, num_steps=NS, noise=noise, guide=guide, use_graph=False, **kw), "graph vs eager")
    assert torch.equal(rec["energy"], model.last_guidance["energy"])
    plain = model.sample(db, num_steps=NS, noise=noise, **kw)
    moving = batch["generate_mask"] & kw["sample_bb"]
    assert not torch.equal(plain[1]["trans"][moving], a[1]["trans"][moving])
    assert torch.equal(plain[1]["trans"][~moving], a[1]["trans"][~moving])


def test_half_batches_equal_the_whole_batch(model):
    NS = CC.NS_E2E
    batch = CC.e2e_batch("L64")
    B, L = batch["aa"].shape
    db = _dev(batch)
    guide = GC.e2e_guide("L64", "b")                          # hot spots [B, L] and one restraint list per sample
    whole = model.sample(db, num_steps=NS, seed=9, guide=guide)
    rec = model.last_guidance
    for lo in range(B):
        sub = {k: v[lo:lo + 1].contiguous() for k, v in db.items()}
        part = model.sample(sub, num_steps=NS, seed=9, first_sample=lo, guide=sampler.shard_guide(guide, lo, lo + 1, B))
        for i in range(NS):
            for k in whole[i]:
                assert torch.equal(part[i][k], whole[i][k][lo:lo + 1]), (lo, i, k)
        assert torch.equal(model.last_guidance["energy"], rec["energy"][:, lo:lo + 1]) and torch.equal(model.last_guidance["shift_max"], rec["shift_max"][:, lo:lo + 1])


def test_ragged_batch_through_the_length_buckets(model):
    """lengths 48, 48, 144, 144: two buckets, each with its samples' own hot spots and restraint lists, against buckets=False; the
    bounds of tests/test_gpu_cond.py's test of the same name"""
    NS, L0, lens = 3, 144, [48, 48, 144, 144]
    items = [synth.make_pocket_batch(1, L0, 9, seed=40 + i, lengths=[n]) for i, n in enumerate(lens)]
    batch = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    B = len(lens)
    noise = synth.make_noise(B, L0, NS, seed=6)
    guide = GC.e2e_guide(None, "b", batch=batch)
    db = _dev(batch)
    one = model.sample(db, num_steps=NS, noise=noise, buckets=False, guide=guide)
    rec_one = model.last_guidance
    two = model.sample(db, num_steps=NS, noise=noise, guide=guide)
    rec_two = model.last_guidance
    assert model.last_buckets == [(2, 48), (2, 144)], model.last_buckets
    assert rec_two["energy"].shape == rec_one["energy"].shape == (NS, B, 5) and float(rec_one["energy"][0].sum(-1).min()) > 0
    ok = batch["res_mask"]
    for i in range(NS):
        assert torch.equal(one[i]["seqs"], two[i]["seqs"]), f"step {i}: sequences differ"
        assert torch.equal(one[i]["seqs_simplex"], two[i]["seqs_simplex"])
        for k in ("rotmats", "trans"):
            e = G.rel_err(two[i][k][ok], one[i][k][ok])
            assert e < 3e-5 * (1 + 3 * i), (i, k, e)
        d = (two[i]["angles"][ok] - one[i]["angles"][ok]).abs()
        assert torch.minimum(d, 2 * math.pi - d).max() < 1e-4 * (1 + 3 * i), (i, "angles")
        for k in ("rotmats", "trans", "angles"):
            assert torch.equal(one[i][k][~ok], two[i][k][~ok]), f"step {i}: padded rows of {k} differ"
    plain = model.sample(db, num_steps=NS, noise=noise)
    assert torch.equal(plain[0]["trans"][ok], two[0]["trans"][ok])              # t = 0.01 < t_on = 0.2: the first step is not guided
    assert not torch.equal(plain[1]["trans"][ok], two[1]["trans"][ok])
