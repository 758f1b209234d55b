"""Conditioned sampling on a real MI355X: partial start, per-residue switches, allowed residue types, free time grid.

Part 1 drives pf_sampler_init_cond / pf_sampler_step_cond through the C ABI alone, on fabricated "network outputs" (tests/cond_cases.py,
milliseconds each); part 2 runs FlowModel.sample end to end against tests/cond_oracle.py.

Tolerances.  Sequences: equal (every case's draws keep a top-2 gap >= 5 % on the oracle's own run).  Rotations 2e-5 max-normalised and
angles 5e-6 wrapped: what test_gpu_parity.test_so3_and_torus_kats holds the same device functions to; rotations are compared where the
relative angle of the geodesic lies in [0.05, pi - 0.1] (cond_oracle.ROT_ANGLE_*: the log map is ill-conditioned at pi).  Translations
and simplex values: 4 x the fp32 oracle's own deviation from the same oracle run in float64 + 1 fp32 ulp of the tensor's largest
magnitude (the rule of tests/test_gpu_optim.py); the measured ratio is printed.  End to end: test_gpu_bigshape._compare_traj and the
bounds of tests/test_gpu_buckets.py."""
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
from pepflowww_amd import _capi, sampler, synth  # noqa: E402
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import gpu_util as G  # noqa: E402
from test_gpu_bigshape import _compare_traj  # noqa: E402

STATE = ("rot_t", "trans_t", "ang_t", "seq_t", "simplex_t", "trans0", "simplex0")
TRAJ = ("traj_rot", "traj_trans", "traj_ang", "traj_seq", "traj_simplex")


def cu(t):
    return t.to(G.dev()).contiguous()


# ==== part 1: the two entry points alone ================================================================================================
class Abi:
    """Device buffers of one fabricated case behind a pf_sampler_args; run() = init + NS steps with the case's predictions copied in."""

    def __init__(self, case, noise, grid, flags=(True, True, True), expo=True, seed=5):
        self.case, self.B, self.L, self.NS = case, case["B"], case["L"], case["NS"]
        rows, NS, dev = self.B * self.L, self.NS, G.dev()
        f = lambda *s: torch.zeros(*s, device=dev)
        i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)
        R1, x1, ang1, seq1 = case["gt"]
        t = self.t = {"rot1": cu(R1.reshape(rows, 9)), "trans1": cu(x1.reshape(rows, 3)), "ang1": cu(ang1.reshape(rows, 5)), "seq1": cu(seq1.reshape(rows)),
                      "gen_mask": cu(case["batch"]["generate_mask"].reshape(rows).float()), "res_mask": cu(case["batch"]["res_mask"].reshape(rows).float()),
                      "rot_t": f(rows, 9), "trans_t": f(rows, 3), "ang_t": f(rows, 5), "seq_t": i64(rows), "simplex_t": f(rows, 20),
                      "trans0": f(rows, 3), "simplex0": f(rows, 20),
                      "pred_rot": f(rows, 9), "pred_trans": f(rows, 3), "pred_ang_raw": f(rows, 5), "pred_logits": f(rows, 20),
                      "traj_rot": f(NS, rows, 9), "traj_trans": f(NS, rows, 3), "traj_ang": f(NS, rows, 5), "traj_seq": i64(NS, rows),
                      "traj_simplex": f(NS, rows, 20), "ts": cu(grid.float()), "step": torch.zeros(2, dtype=torch.int32, device=dev), "t_out": f(self.B)}
        assert t["ts"].shape == (NS,)
        self.noise = {k: cu(noise[k].reshape(rows, -1)) for k in ("rot0", "trans0", "ang0", "simplex0")}
        a = self.args = _capi.SamplerArgs()
        for k, v in t.items():
            setattr(a, k, v.data_ptr())
        if expo:
            assert noise["expo"].shape == (2 * NS, self.B, self.L, 20)
            self.expo = cu(noise["expo"])
            a.expo = self.expo.data_ptr()
        a.num_steps, a.B, a.L, a.seed, a.first_sample = NS, self.B, self.L, seed, 3
        a.sample_bb, a.sample_ang, a.sample_seq = (int(x) for x in flags)
        self.keep = []

    def cond(self, flags=None, aa_allowed=None, start=None):
        """pf_sampler_cond_args of cond_oracle.sample's keywords (flags: three bools / bool [B, L] tensors, or a ready uint8 plane)"""
        B, L, rows = self.B, self.L, self.B * self.L
        c = _capi.SamplerCondArgs()
        if flags is not None:
            plane = flags if torch.is_tensor(flags) and flags.dtype == torch.uint8 else sampler.pack_res_flags(*flags, B, L)[1]
            if plane is not None:
                self.keep.append(cu(plane.reshape(rows)))
                c.res_flags = self.keep[-1].data_ptr()
        if aa_allowed is not None:
            self.keep.append(cu(sampler.pack_aa_allowed(aa_allowed, B, L).reshape(rows)))
            c.aa_allowed = self.keep[-1].data_ptr()
        if start is not None:
            c.partial = 1
            for name, key, w in (("start_rot", "rotmats", 9), ("start_trans", "trans", 3), ("start_ang", "angles", 5), ("start_seq", "seqs", 1)):
                self.keep.append(cu(start[key].reshape(rows, w)))
                setattr(c, name, self.keep[-1].data_ptr())
        return c

    def run(self, entry="cond", cond=None):
        lib, a, t, nz = _capi.load(), self.args, self.t, self.noise
        for k in STATE + TRAJ:
            t[k].fill_(-7)                          # (whatever an earlier run left)
        cp = None if cond is None else C.byref(cond)
        st = _capi.stream_ptr()
        noise_ptrs = (nz["rot0"].data_ptr(), nz["trans0"].data_ptr(), nz["ang0"].data_ptr(), nz["simplex0"].data_ptr())
        if entry == "plain":
            _capi.check(lib.pf_sampler_init(C.byref(a), *noise_ptrs, st), "pf_sampler_init")
        else:
            _capi.check(lib.pf_sampler_init_cond(C.byref(a), cp, *noise_ptrs, st), "pf_sampler_init_cond")
        snap = lambda: {k: t[k].cpu().clone() for k in STATE}
        out = {"init": snap(), "states": [], "t_out": [t["t_out"].cpu().clone()]}
        for s in range(self.NS):
            for k, v in zip(("pred_rot", "pred_trans", "pred_ang_raw", "pred_logits"), self.case["preds"][s]):
                t[k].copy_(v.reshape(t[k].shape))
            if entry == "plain":
                _capi.check(lib.pf_sampler_step(C.byref(a), st), "pf_sampler_step")
            else:
                _capi.check(lib.pf_sampler_step_cond(C.byref(a), cp, st), "pf_sampler_step_cond")
            out["states"].append(snap())
            out["t_out"].append(t["t_out"].cpu().clone())
        out["traj"] = {k: t[k].cpu().clone() for k in TRAJ}
        assert t["step"].tolist() == [self.NS, 0]
        return out


def assert_same_run(a, b, what):
    for k in STATE:
        assert torch.equal(a["init"][k], b["init"][k]), (what, "init", k)
        for s, (x, y) in enumerate(zip(a["states"], b["states"])):
            assert torch.equal(x[k], y[k]), (what, "state", s, k)
    for k in TRAJ:
        assert torch.equal(a["traj"][k], b["traj"][k]), (what, k)
    for x, y in zip(a["t_out"], b["t_out"]):
        assert torch.equal(x, y), (what, "t_out")


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_null_and_empty_cond_are_the_unconstrained_kernels(shape):
    case = CC.abi_case(shape)
    for flags in ((True, True, True), (True, False, True)):
        h = Abi(case, case["noise"], CO.make_grid(case["NS"]), flags)
        plain = h.run("plain")
        assert torch.isfinite(plain["traj"]["traj_rot"]).all() and (plain["traj"]["traj_seq"] >= 0).all()
        assert_same_run(plain, h.run("cond", None), "cond = NULL")
        assert_same_run(plain, h.run("cond", _capi.SamplerCondArgs()), "empty struct")


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_constant_plane_equals_the_scalar_flags(shape):
    """all eight combinations, on every row (generated or not); the scalar fields are set to the OPPOSITE while the plane is in charge.
    With all 20 classes allowed on top, the masked draws resolve every rounding and tie as the unmasked ones: the same bits."""
    case = CC.abi_case(shape)
    grid = CO.make_grid(case["NS"])
    every = torch.ones(20, dtype=torch.bool)
    for bits in range(8):
        flags = tuple(bool(bits >> k & 1) for k in range(3))
        plain = Abi(case, case["noise"], grid, flags).run("plain")
        h = Abi(case, case["noise"], grid, tuple(not f for f in flags))
        plane = torch.full((case["B"], case["L"]), bits, dtype=torch.uint8)
        assert_same_run(plain, h.run("cond", h.cond(flags=plane)), f"plane {bits}")
        assert_same_run(plain, h.run("cond", h.cond(flags=plane, aa_allowed=every)), f"plane {bits} + all classes")
    h = Abi(case, case["noise"], grid)
    assert_same_run(Abi(case, case["noise"], grid).run("plain"), h.run("cond", h.cond(aa_allowed=every)), "all classes alone")


def _wrapped(a, b):
    d = (a.double() - b.double()).abs()
    return float(torch.minimum(d, 2 * math.pi - d).max())


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _f64_rule(got, ref32, ref64, what, ratios):
    """|kernel - float64 oracle| <= 4 x |fp32 oracle - float64 oracle| + 1 fp32 ulp of the largest magnitude, per tensor"""
    d_k = float((got.double() - ref64).abs().max())
    d_r = float((ref32.double() - ref64).abs().max())
    tol = 4.0 * d_r + _ulp32(float(ref64.abs().max()))
    ratios.append((d_k / tol, what, d_k, d_r, tol))
    assert d_k <= tol, (what, d_k, d_r, tol)


def _check_state(got, ref32, ref64, rot_rows, what, ratios, L):
    """one state (rot, trans, angles, seq, simplex) of the device against the oracle's, by the rules in the module docstring"""
    B = ref32[0].shape[0]
    assert torch.equal(got["seq_t"].view(B, L), ref32[3]), f"{what}: sequences differ"
    R = got["rot_t"].view(B, L, 3, 3)
    assert rot_rows.any()
    G.assert_close(R[rot_rows], ref32[0][rot_rows], 2e-5, f"{what} rotations")
    assert _wrapped(got["ang_t"].view(B, L, 5), ref32[2]) < 5e-6, f"{what} angles"
    _f64_rule(got["trans_t"].view(B, L, 3), ref32[1], ref64[1], f"{what} trans", ratios)
    _f64_rule(got["simplex_t"].view(B, L, 20), ref32[4], ref64[4], f"{what} simplex", ratios)


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", ["partial_t001", "partial_t05", "partial_t099"])
def test_partial_init_vs_oracle(shape, name):
    c = CC.abi_config(shape, name)
    case, kw = c["case"], c["kw"]
    B, L, NS = case["B"], case["L"], case["NS"]
    o = dict(encoded=case["encoded"], preds=case["preds"], init_only=True, **kw)
    ref32 = CO.sample(None, case["batch"], c["noise"], NS, **o)
    ref64 = CO.sample(None, case["batch"], c["noise"], NS, dtype=torch.float64, **o)
    h = Abi(case, c["noise"], CO.make_grid(NS, kw["t_start"]))
    got = h.run("cond", h.cond(start=kw["start"]))["init"]
    ratios = []
    _check_state(got, ref32, ref64, torch.ones(B, L, dtype=torch.bool), name, ratios, L)
    _f64_rule(got["trans0"].view(B, L, 3), ref32[5], ref64[5], "trans0", ratios)          # the noise kept for the Euler steps: as pf_sampler_init
    _f64_rule(got["simplex0"].view(B, L, 20), ref32[6], ref64[6], "simplex0", ratios)
    gen = case["batch"]["generate_mask"]
    if kw["t_start"] == 0.5:                      # ... and the state really is between the noise and the start
        assert (got["trans_t"].view(B, L, 3)[gen] - got["trans0"].view(B, L, 3)[gen]).abs().max() > 0.1
    print(f"{shape} {name}: worst kernel deviation / tolerance = {max(ratios)[0]:.3f} ({max(ratios)[1]})")


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", ["mixed_one", "mixed_no_cys", "mixed_random", "nonuniform_ts"])
def test_flags_allowed_sets_and_grid_vs_oracle(shape, name):
    """mixed per-row flags with allowed sets of one class, of 19 classes (no CYS) and random ones; a non-uniform grid: trajectory and the
    state after every Euler step against the oracle, zero flipped draws"""
    c = CC.abi_config(shape, name)
    case, kw, ref = c["case"], c["kw"], c["ref"]
    B, L, NS = case["B"], case["L"], case["NS"]
    s32, s64 = [], []
    o = dict(encoded=case["encoded"], preds=case["preds"], **kw)
    CO.sample(None, case["batch"], c["noise"], NS, states=s32, **o)
    CO.sample(None, case["batch"], c["noise"], NS, states=s64, dtype=torch.float64, **o)
    grid = CO.make_grid(NS, kw["t_start"], kw["ts"])
    h = Abi(case, c["noise"], grid)
    got = h.run("cond", h.cond(flags=kw["flags"], aa_allowed=kw["aa_allowed"], start=kw["start"]))
    tr = got["traj"]
    for i in range(NS):
        assert torch.equal(tr["traj_seq"][i].view(B, L), ref[i]["seqs"]), f"step {i}: flipped draws"
        assert torch.equal(tr["traj_simplex"][i].view(B, L, 20), ref[i]["seqs_simplex"])
        assert torch.equal(tr["traj_rot"][i].view(B, L, 3, 3), ref[i]["rotmats"]) and torch.equal(tr["traj_trans"][i].view(B, L, 3), ref[i]["trans"])
        assert _wrapped(tr["traj_ang"][i].view(B, L, 5), ref[i]["angles"]) < 5e-6, f"step {i} angles"
        assert torch.equal(got["t_out"][i], grid[i].expand(B))
    ratios = []
    ok = torch.ones(B, L, dtype=torch.bool)
    fb = CO.row_flags(kw["flags"], case["batch"]["generate_mask"])[0]
    moving = case["batch"]["generate_mask"] & fb               # the rows whose rotation takes geodesic steps at all
    for s in range(NS - 1):
        ok = ok & s32[s][5]
        _check_state(got["states"][s], s32[s], s64[s], ok, f"{name} state {s}", ratios, L)
        # The band is a condition of comparing a geodesic's result, here as at the init; it must not hollow the check out.  The
        # predicted rotations are Haar-random, so a step's relative angle has density (1 - cos x) / pi: 6.4 % of the rows leave the
        # band per step (x > pi - 0.1; x < 0.05 is 1e-5), 12 % over the two steps -- at least half of the moving rows must remain.
        n_ok, n_mv = int((ok & moving).sum()), int(moving.sum())
        print(f"{shape} {name} state {s}: rotations compared on {n_ok} of {n_mv} moving rows")
        assert n_mv >= 4 and n_ok >= 0.5 * n_mv, (s, n_ok, n_mv)
    assert_same_run({**got, "states": got["states"][-1:]}, {**got, "states": got["states"][-2:-1]}, "the last step only records")
    print(f"{shape} {name}: worst kernel deviation / tolerance = {max(ratios)[0]:.3f} ({max(ratios)[1]})")


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", ["mixed_one", "mixed_no_cys", "mixed_random"])
def test_philox_draws_stay_in_the_allowed_set(shape, name):
    """expo = NULL: the in-kernel Philox draws, for the same three kinds of sets; every drawn residue type of a row that samples its
    sequence lies in the row's set, and two runs are bit-equal.  (The one-class and random sets exclude half or more of the classes on
    every row, so some draw of the unmasked run must change; excluding CYS alone need not change any draw, so that is not asserted.)"""
    c = CC.abi_config(shape, name)
    case, kw = c["case"], c["kw"]
    B, L, NS = case["B"], case["L"], case["NS"]
    h = Abi(case, c["noise"], CO.make_grid(NS, kw["t_start"], kw["ts"]), expo=False)
    cond = h.cond(flags=kw["flags"], aa_allowed=kw["aa_allowed"], start=kw["start"])
    one, two = h.run("cond", cond), h.run("cond", cond)
    assert_same_run(one, two, "repeat")
    rows = case["batch"]["generate_mask"] & kw["flags"][2]
    allowed = CO.allowed_rows(kw["aa_allowed"], B, L)
    seqs = [one["init"]["seq_t"]] + [s["seq_t"] for s in one["states"]] + list(one["traj"]["traj_seq"])
    assert rows.sum() > 3
    for q in seqs:
        q = q.view(B, L)
        assert allowed[rows].gather(-1, q[rows][:, None]).all()
        assert torch.equal(q[~rows], case["gt"][3][~rows])
    free = Abi(case, c["noise"], CO.make_grid(NS, kw["t_start"], kw["ts"]), expo=False)
    other = free.run("cond", free.cond(flags=kw["flags"], start=kw["start"]))
    if name != "mixed_no_cys":
        assert not torch.equal(other["traj"]["traj_seq"], one["traj"]["traj_seq"]), "the mask must change some draw"


# ==== part 2: FlowModel.sample ==========================================================================================================
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


@pytest.mark.parametrize("shape", list(CC.E2E_SHAPES))
def test_default_grid_and_no_leak_from_a_conditioned_call(model, shape):
    """t_start = 1e-2 is the plain call; a plain call after conditioned calls (another grid, constraint planes, a partial start) at the
    same shape gets the bits of the one before them; graph replay equals eager launches under every new argument."""
    batch = CC.e2e_batch(shape)
    B, L = batch["aa"].shape
    NS = CC.NS_E2E
    noise = synth.make_noise(B, L, NS, seed=5)
    db = _dev(batch)
    before = model.sample(db, num_steps=NS, noise=noise)
    _same_traj(before, model.sample(db, num_steps=NS, noise=noise, t_start=1e-2), "t_start = 1e-2")
    shifted = model.sample(db, num_steps=NS, noise=noise, t_start=0.7)                     # the plain sampler on another grid
    assert not torch.equal(shifted[1]["trans"], before[1]["trans"])
    g = torch.Generator().manual_seed(3)
    kw = CC.sample_kwargs({"flags": CC._mixed_flags(B, L, g), "aa_allowed": CC._allowed("random", B, L, g), "ts": [0.2, 0.5, 0.6, 1.0], "start": "native"})
    graph = model.sample(db, num_steps=NS, noise=noise, **kw)
    eager = model.sample(db, num_steps=NS, noise=noise, use_graph=False, **kw)
    _same_traj(graph, eager, "graph replay vs eager")
    assert not torch.equal(graph[0]["trans"], before[0]["trans"])
    _same_traj(before, model.sample(db, num_steps=NS, noise=noise), "plain call after conditioned calls")
    _same_traj(graph, model.sample(db, num_steps=NS, noise=noise, **kw), "conditioned call after a plain call")


@pytest.mark.parametrize("shape", list(CC.E2E_SHAPES))
@pytest.mark.parametrize("name", CC.E2E_CONFIGS)
def test_sample_vs_oracle(model, seeded_sd, shape, name):
    NS = CC.NS_E2E
    batch = CC.e2e_batch(shape)
    db = _dev(batch)
    start = None
    if name == "traj_start":                       # start = traj[-1] of a first run ON THE DEVICE; the oracle is given the same state
        L = batch["aa"].shape[1]
        start = model.sample(db, num_steps=NS, noise=synth.make_noise(CC.B_E2E, L, NS, seed=31 + CC.E2E_CONFIGS.index(name)))[-1]
    c = CC.e2e_config(seeded_sd, shape, name, start=start)
    rec = []
    with torch.no_grad():
        ref = CO.sample(seeded_sd, batch, c["noise"], NS, encoded=c["encoded"], rec=rec, **c["kw"])
    assert CO.min_gap(rec, batch["generate_mask"]) >= CO.DRAW_GAP
    kw = CC.sample_kwargs(c["kw"])
    if name == "traj_start":
        kw["start"] = start                        # the trajectory dict itself (CPU tensors, further keys ignored)
    traj = model.sample(db, num_steps=NS, noise=c["noise"], **kw)
    _compare_traj(traj, ref, 0, CC.B_E2E, NS, f"{shape} {name}")
    gen = batch["generate_mask"]
    if "aa_allowed" in kw:
        rows = gen & c["kw"]["flags"][2]
        for t in traj:
            assert c["kw"]["aa_allowed"][rows].gather(-1, t["seqs"][rows][:, None]).all()
    plain = model.sample(db, num_steps=NS, noise=c["noise"])
    assert not torch.equal(plain[0]["trans"][gen], traj[0]["trans"][gen]), "the conditioning must change the run"


def test_device_tensors_are_accepted(model):
    """start / flags / aa_allowed given as DEVICE tensors at L0 = 24 (padded to 32 on the device) give the bits of the same call with CPU
    tensors; a start with a residue type that is none raises before anything runs"""
    NS = CC.NS_E2E
    batch = CC.e2e_batch("L24")
    B, L = batch["aa"].shape
    db = _dev(batch)
    noise = synth.make_noise(B, L, NS, seed=8)
    first = model.sample(db, num_steps=NS, noise=noise)[-1]
    g = torch.Generator().manual_seed(4)
    start = {k: first[k].clone() for k in ("rotmats", "trans", "angles", "seqs")}
    flags, allowed = CC._mixed_flags(B, L, g), CC._allowed("random", B, L, g)
    host = model.sample(db, num_steps=NS, noise=noise, t_start=0.5, start=start, aa_allowed=allowed, sample_bb=flags[0], sample_seq=flags[2])
    dev = model.sample(db, num_steps=NS, noise=noise, t_start=0.5, start={k: cu(v) for k, v in start.items()}, aa_allowed=cu(allowed),
                       sample_bb=cu(flags[0]), sample_seq=cu(flags[2]))
    _same_traj(host, dev, "device tensors")
    assert not torch.equal(host[0]["trans"], model.sample(db, num_steps=NS, noise=noise, t_start=0.5)[0]["trans"])
    bad = cu(start["seqs"].clone())
    bad[0, 0] = 22
    with pytest.raises(ValueError, match="0..21"):
        model.sample(db, num_steps=NS, noise=noise, t_start=0.5, start={"seqs": bad})


def test_half_batches_equal_the_whole_batch(model):
    """Philox draws and seeded noise (noise = None, explicit seed), every new argument set: two shards of one sample each with
    first_sample = 0 / 1 reproduce the whole batch bit for bit"""
    NS = CC.NS_E2E
    batch = CC.e2e_batch("L64")
    B, L = batch["aa"].shape
    db = _dev(batch)
    g = torch.Generator().manual_seed(11)
    first = model.sample(db, num_steps=NS, seed=5)[-1]
    flags = CC._mixed_flags(B, L, g)
    allowed = CC._allowed("random", B, L, g)
    start = {k: first[k] for k in ("rotmats", "trans", "seqs")}                            # (angles: the native's)
    whole = model.sample(db, num_steps=NS, seed=9, t_start=0.3, start=start, aa_allowed=allowed,
                         sample_bb=flags[0], sample_ang=flags[1], sample_seq=flags[2])
    rows = batch["generate_mask"] & flags[2]
    assert allowed[rows].gather(-1, whole[-1]["seqs"][rows][:, None]).all()
    for lo in range(B):
        sub = {k: v[lo:lo + 1].contiguous() for k, v in db.items()}
        part = model.sample(sub, num_steps=NS, seed=9, first_sample=lo, t_start=0.3, start={k: v[lo:lo + 1] for k, v in start.items()},
                            aa_allowed=allowed[lo:lo + 1], sample_bb=flags[0][lo:lo + 1], sample_ang=flags[1][lo:lo + 1], sample_seq=flags[2][lo:lo + 1])
        for i in range(NS):
            for k in whole[i]:
                assert torch.equal(part[i][k], whole[i][k][lo:lo + 1]), (lo, i, k)


def test_ragged_batch_through_the_length_buckets(model):
    """lengths 48, 48, 144, 144: two buckets with their own engines, samplers, constraint planes and start states (and the conditioned
    init re-run after the stream calibration's probe steps) against buckets=False; bounds of tests/test_gpu_buckets.py"""
    NS, L0, lens = 3, 144, [48, 48, 144, 144]
    items = [synth.make_pocket_batch(1, L0, 9, seed=40 + i, lengths=[n]) for i, n in enumerate(lens)]
    batch = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    B = len(lens)
    noise = synth.make_noise(B, L0, NS, seed=6)
    g = torch.Generator().manual_seed(2)
    kw = CC.sample_kwargs({"flags": CC._mixed_flags(B, L0, g), "aa_allowed": CC._allowed("random", B, L0, g), "t_start": 0.5, "start": "native"})
    db = _dev(batch)
    one = model.sample(db, num_steps=NS, noise=noise, buckets=False, **kw)
    two = model.sample(db, num_steps=NS, noise=noise, **kw)
    assert model.last_buckets == [(2, 48), (2, 144)], model.last_buckets
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
    assert not torch.equal(plain[0]["trans"][ok], two[0]["trans"][ok])
