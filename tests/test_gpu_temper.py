"""Tempered and stochastic sampling on a real MI355X: pf_sampler_temper in front of pf_sampler_step_cond on fabricated "network outputs"
(through the C ABI), the kernel alone with its own Philox draws, and end to end through FlowModel.sample(temper=...).

Tolerances: the rules of tests/test_gpu_cond.py, imported and unchanged.  Sequences and simplex records equal (every case's draws keep a
top-2 gap >= 5 % on the temper oracle's own run, tests/temper_cases.py); rotations 2e-5 max-normalised where the geodesic's relative
angle lies in cond_oracle's band; angles 5e-6 wrapped; translations and simplex values by _f64_rule (4 x the fp32 oracle's own deviation
from the float64 oracle + 1 fp32 ulp).  The in-kernel normals are held to the same rule against tests/temper_oracle.py's integer
restatement of the counter layout: its float32 variant against its float64 variant.  End to end: test_gpu_bigshape._compare_traj and
the bounds of test_gpu_cond's ragged test.  The conditions the cases must meet are asserted on the CPU in tests/test_temper_cpu.py."""
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
import guide_cases as GC  # noqa: E402
import temper_cases as TC  # noqa: E402
import temper_oracle as TO  # noqa: E402
import gpu_util as G  # noqa: E402
from cond_oracle import O  # noqa: E402
from test_gpu_bigshape import _compare_traj  # noqa: E402
from test_gpu_cond import STATE, TRAJ, Abi, _check_state, _f64_rule, _wrapped, assert_same_run, cu  # noqa: E402

SENTINEL = -7.0
PRED = ("pred_rot", "pred_trans", "pred_ang_raw", "pred_logits")


# ==== the kernel in front of the step kernel, through the C ABI =========================================================================
class Temper:
    """device buffers of one pf_sampler_temper_args on top of an Abi's state: the network's logits go to `raw`, the step kernel reads
    `tempered` when a temperature plane is given and `raw` otherwise"""

    def __init__(self, h, temper, cond, gauss):
        B, L, NS = h.B, h.L, h.NS
        rows, dev = B * L, G.dev()
        self.packed = sampler.make_temper(temper, B, L)
        self.raw = torch.zeros(rows, 20, device=dev)
        self.tempered = torch.full((rows, 20), SENTINEL, device=dev)
        self.params = cu(self.packed["params"])
        a = self.args = _capi.SamplerTemperArgs()
        a.pred_logits, a.tempered_logits = self.raw.data_ptr(), self.tempered.data_ptr()
        self.tau = None
        if self.packed["tau"] is not None:
            self.tau = cu(self.packed["tau"].reshape(rows))
            a.tau = self.tau.data_ptr()
        self.logits_for_step = self.tempered if self.tau is not None else self.raw
        a.rot_t, a.trans_t, a.gen_mask = h.t["rot_t"].data_ptr(), h.t["trans_t"].data_ptr(), h.t["gen_mask"].data_ptr()
        a.res_flags = cond.res_flags
        a.ts, a.step, a.params = h.t["ts"].data_ptr(), h.t["step"].data_ptr(), self.params.data_ptr()
        self.gauss = None
        if gauss is not None:
            assert gauss.shape == (NS - 1, B, L, 6)
            self.gauss = cu(gauss)
            a.gauss = self.gauss.data_ptr()
        a.seed, a.first_sample = h.args.seed, h.args.first_sample
        a.B, a.L, a.num_steps, a.sample_bb = B, L, NS, 0           # (the plane is in charge: the scalar says the opposite)

    def launch(self):
        _capi.check(_capi.load().pf_sampler_temper(C.byref(self.args), _capi.stream_ptr()), "pf_sampler_temper")


def _run(h, cond, tp=None):
    """init + NS x (copy the case's predictions in, [pf_sampler_temper,] pf_sampler_step_cond); -> the keys of Abi.run plus, per step,
    the state before and after the temper kernel and the tempered buffer it left"""
    lib, a, t, nz, st = _capi.load(), h.args, h.t, h.noise, _capi.stream_ptr()
    for k in STATE + TRAJ:
        t[k].fill_(SENTINEL)
    logits_in = t["pred_logits"] if tp is None else tp.raw
    a.pred_logits = (t["pred_logits"] if tp is None else tp.logits_for_step).data_ptr()
    _capi.check(lib.pf_sampler_init_cond(C.byref(a), C.byref(cond), nz["rot0"].data_ptr(), nz["trans0"].data_ptr(), nz["ang0"].data_ptr(),
                                         nz["simplex0"].data_ptr(), st), "pf_sampler_init_cond")
    snap = lambda: {k: t[k].cpu().clone() for k in STATE}  # noqa: E731
    out = {"init": snap(), "states": [], "t_out": [t["t_out"].cpu().clone()], "before": [], "after": [], "tempered": []}
    for s in range(h.NS):
        for buf, v in zip((t["pred_rot"], t["pred_trans"], t["pred_ang_raw"], logits_in), h.case["preds"][s]):
            buf.copy_(v.reshape(buf.shape))
        if tp is not None:
            tp.tempered.fill_(SENTINEL)
            out["before"].append(snap())
            tp.launch()
            out["after"].append(snap())
            out["tempered"].append(tp.tempered.cpu().clone())
        _capi.check(lib.pf_sampler_step_cond(C.byref(a), C.byref(cond), st), "pf_sampler_step_cond")
        out["states"].append(snap())
        out["t_out"].append(t["t_out"].cpu().clone())
    out["traj"] = {k: t[k].cpu().clone() for k in TRAJ}
    assert t["step"].tolist() == [h.NS, 0]
    return out


def _device_run(c, with_kernel=True, temper=None, gauss=True):
    case, kw = c["case"], c["kw"]
    grid = CO.make_grid(case["NS"], kw.get("t_start"), kw.get("ts"))
    h = Abi(case, c["noise"], grid)
    cond = h.cond(flags=kw["flags"])
    tp = Temper(h, c["temper"] if temper is None else temper, cond, c["noise"]["gauss"] if gauss else None) if with_kernel else None
    return _run(h, cond, tp), h, tp, grid


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", TC.ALL_CONFIGS)
def test_temper_then_step_kernel_vs_oracle(shape, name):
    """trajectory and the state after every Euler step against temper_oracle.sample on the same supplied normals"""
    c = TC.abi_config(shape, name)
    case, kw, ref = c["case"], c["kw"], c["ref"]
    B, L, NS = case["B"], case["L"], case["NS"]
    s32, s64 = [], []
    o = dict(temper=c["temper"], encoded=case["encoded"], preds=case["preds"], **kw)
    TO.sample(None, case["batch"], c["noise"], NS, states=s32, **o)
    TO.sample(None, case["batch"], c["noise"], NS, states=s64, dtype=torch.float64, **o)
    got, _, _, grid = _device_run(c)
    tr = got["traj"]
    for i in range(NS):
        assert torch.equal(tr["traj_seq"][i].view(B, L), ref[i]["seqs"]), f"step {i}: flipped draws"
        assert torch.equal(tr["traj_simplex"][i].view(B, L, 20), ref[i]["seqs_simplex"])
        assert torch.equal(tr["traj_rot"][i].view(B, L, 3, 3), ref[i]["rotmats"]) and torch.equal(tr["traj_trans"][i].view(B, L, 3), ref[i]["trans"])
        assert _wrapped(tr["traj_ang"][i].view(B, L, 5), ref[i]["angles"]) < 5e-6, f"step {i} angles"
        assert torch.equal(got["t_out"][i], grid[i].expand(B))
    ratios = []
    ok = torch.ones(B, L, dtype=torch.bool)
    moving = TC.movable(case)
    for s in range(NS - 1):
        ok = ok & s32[s][5]
        _check_state(got["states"][s], s32[s], s64[s], ok, f"{name} state {s}", ratios, L)
        n_ok, n_mv = int((ok & moving).sum()), int(moving.sum())
        print(f"{shape} {name} state {s}: rotations compared on {n_ok} of {n_mv} moving rows")
        assert n_mv >= 4 and n_ok >= 0.5 * n_mv, (s, n_ok, n_mv)            # (the band must not hollow the check out: test_gpu_cond)
    assert_same_run({**got, "states": got["states"][-1:]}, {**got, "states": got["states"][-2:-1]}, "the last step only records")
    print(f"{shape} {name}: worst kernel deviation / tolerance = {max(ratios)[0]:.3f} ({max(ratios)[1]})")


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_unit_temperature_and_zero_sigmas_are_the_run_without_the_kernel(shape):
    c = TC.abi_config(shape, "full")
    case = c["case"]
    plain, _, _, _ = _device_run(c, with_kernel=False)
    ones = {"seq_temperature": torch.ones(case["B"], case["L"]), "sigma_trans": 0.0, "sigma_rot": 0.0}
    got, _, tp, _ = _device_run(c, temper=ones)
    assert tp.tau is not None
    assert_same_run(plain, got, "tau = 1, sigma = 0")
    for s in range(case["NS"]):                                            # ... and the division by one gives back the input's bits
        assert torch.equal(got["tempered"][s], case["preds"][s][3].reshape(-1, 20))
    tempered, _, _, _ = _device_run(c)
    assert not torch.equal(tempered["traj"]["traj_seq"], plain["traj"]["traj_seq"]) and not torch.equal(tempered["states"][0]["trans_t"], plain["states"][0]["trans_t"])


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_the_kernel_writes_what_it_owns_and_nothing_else(shape):
    c = TC.abi_config(shape, "full")
    case = c["case"]
    B, L, NS = case["B"], case["L"], case["NS"]
    mov = TC.movable(case).reshape(-1)
    assert mov.any() and (~mov).any()
    got, h, tp, _ = _device_run(c)
    tau = tp.packed["tau"].reshape(-1, 1)
    for s in range(NS):
        b, a = got["before"][s], got["after"][s]
        assert (got["tempered"][s] != SENTINEL).all(), f"step {s}: a sentinel survived in tempered_logits"
        assert torch.equal(got["tempered"][s], case["preds"][s][3].reshape(-1, 20) / tau), "all 20 classes of every row, every step"
        for k in ("ang_t", "seq_t", "simplex_t", "trans0", "simplex0"):
            assert torch.equal(b[k], a[k]), (s, k)
        for k in ("rot_t", "trans_t"):
            assert torch.equal(b[k][~mov], a[k][~mov]), (s, k, "rows that do not move keep their bits")
            if s < NS - 1:
                assert (b[k][mov] != a[k][mov]).any(-1).all(), (s, k, "every movable row is perturbed")
            else:
                assert torch.equal(b[k], a[k]), (k, "the record-only last step gets no noise")
    # *step >= num_steps: returns without writing anything
    tp.tempered.fill_(SENTINEL)
    keep = {k: h.t[k].clone() for k in STATE}
    assert h.t["step"].tolist() == [NS, 0]
    tp.launch()
    assert (tp.tempered == SENTINEL).all() and all(torch.equal(keep[k], h.t[k]) for k in STATE)
    # tau = NULL: the buffer is never written, and the step kernel reads the logits themselves
    n = TC.abi_config(shape, "null_plane")
    got, _, tp, _ = _device_run(n)
    assert tp.tau is None and all((x == SENTINEL).all() for x in got["tempered"])
    assert not torch.equal(got["before"][0]["trans_t"][mov], got["after"][0]["trans_t"][mov])
    for k in STATE:                                                        # beyond t_off the whole state keeps its bits
        assert torch.equal(got["before"][1][k], got["after"][1][k]), k


# ==== the kernel alone: its own draws ===================================================================================================
def _draw(B, L, NS, step, movable_rows=None, seed=5, first_sample=0, ids=None, seed_dev=None, sigma=(1.0, 0.0), grid=None):
    """pf_sampler_temper alone on trans_t = 0 and rot_t = identity, power = 0, gauss = NULL -> (trans_t [B,L,3], rot_t [B,L,3,3]) on the CPU"""
    rows, dev = B * L, G.dev()
    mov = torch.ones(B, L, dtype=torch.bool) if movable_rows is None else movable_rows
    keep = {"rot_t": torch.eye(3, device=dev).reshape(1, 9).repeat(rows, 1).contiguous(), "trans_t": torch.zeros(rows, 3, device=dev),
            "gen_mask": cu(mov.reshape(rows).float()), "ts": cu((CO.make_grid(NS) if grid is None else grid).float()),
            "step": torch.tensor([step, 0], dtype=torch.int32, device=dev),
            "params": cu(sampler.make_temper({"sigma_trans": sigma[0], "sigma_rot": sigma[1], "power": 0}, B, L)["params"])}
    a = _capi.SamplerTemperArgs()
    for k, v in keep.items():
        setattr(a, k, v.data_ptr())
    if ids is not None:
        keep["ids"] = cu(torch.as_tensor(ids, dtype=torch.int64))
        a.sample_ids = keep["ids"].data_ptr()
    if seed_dev is not None:
        keep["seed_dev"] = cu(torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seed_dev], dtype=torch.int64))
        a.seed_dev = keep["seed_dev"].data_ptr()
    a.seed, a.first_sample, a.B, a.L, a.num_steps, a.sample_bb = seed, first_sample, B, L, NS, 1
    _capi.check(_capi.load().pf_sampler_temper(C.byref(a), _capi.stream_ptr()), "pf_sampler_temper")
    return keep["trans_t"].cpu().view(B, L, 3), keep["rot_t"].cpu().view(B, L, 3, 3)


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_in_kernel_draws_vs_the_integer_restatement(shape):
    case = TC.abi_case(shape)
    B, L, NS = case["B"], case["L"], 5
    mov = TC.movable(case)
    seed = (5 << 32) | 17                                                  # both words of the key ...
    ids = [(1 << 32) + 7 * b for b in range(B)]                            # ... and of the global sample index are in use
    grid = CO.make_grid(NS)
    eye = torch.eye(3).expand(B, L, 3, 3)
    ratios = []
    for step in (0, NS - 2):
        z32, z64 = (torch.from_numpy(TO.normals(seed, ids, L, step, dt)) for dt in (np.float32, np.float64))
        a32, a64 = (TO.noise_scale(grid, step, {"power": 0}, dt) for dt in (torch.float32, torch.float64))
        sig = torch.tensor(1.5, dtype=torch.float32)
        x, R = _draw(B, L, NS, step, mov, seed, ids=ids, sigma=(1.5, 0.0))
        _f64_rule(x[mov], (sig * a32) * z32[..., 0:3][mov], (sig.double() * a64) * z64[..., 0:3][mov], f"{shape} step {step} sigma a z", ratios)
        assert float(x[~mov].abs().max()) == 0 and torch.equal(R, eye), "rows that do not move, and the rotations of a translation-only run"
        sig = torch.tensor(0.7, dtype=torch.float32)
        x, R = _draw(B, L, NS, step, mov, seed, ids=ids, sigma=(0.0, 0.7))
        G.assert_close(R[mov], O.so3_exp((sig * a32) * z32[..., 3:6])[mov], 2e-5, f"{shape} step {step} Exp(sigma a z)")
        assert torch.equal(R[~mov], eye[~mov]) and float(x.abs().max()) == 0
        assert float((R[mov] - eye[mov]).abs().max()) > 0.1
    print(f"{shape}: worst kernel deviation / tolerance = {max(ratios)[0]:.3f} ({max(ratios)[1]})")
    late = _draw(B, L, NS, NS - 1, mov, seed, ids=ids, sigma=(1.5, 0.7))    # the last step and beyond: no noise
    assert float(late[0].abs().max()) == 0 and torch.equal(late[1], eye)


def test_in_kernel_draws_are_keyed_by_seed_step_and_global_sample():
    B, L, NS = 4, 272, 5
    ids = [10, 11, 12, 13]
    g = lambda **kw: _draw(B, L, NS, kw.pop("step", 1), sigma=(1.0, 0.5), **kw)  # noqa: E731
    x, R = g(seed=9, ids=ids)
    again = g(seed=9, ids=ids)
    assert torch.equal(x, again[0]) and torch.equal(R, again[1])
    rows = x.reshape(-1, 3)
    assert len({tuple(r) for r in rows.tolist()}) == rows.shape[0], "every row draws its own normals"
    for other in (g(seed=10, ids=ids), g(seed=9 + (1 << 32), ids=ids), g(seed=9, ids=ids, step=2)):
        assert (other[0] != x).any(-1).all() and (other[1] != R).flatten(2).any(-1).all()
    one = g(seed=9, ids=[10, 11, 99, 13])                                  # another sample_ids entry: that sample's draws, no other's
    assert torch.equal(one[0][[0, 1, 3]], x[[0, 1, 3]]) and (one[0][2] != x[2]).any(-1).all()
    perm = [2, 0, 3, 1]
    p = g(seed=9, ids=[ids[i] for i in perm])                              # a permuted sample_ids permutes the draws
    assert torch.equal(p[0], x[perm]) and torch.equal(p[1], R[perm])
    f = g(seed=9, first_sample=10)                                         # sample_ids = NULL: first_sample + b
    assert torch.equal(f[0], x) and torch.equal(f[1], R)
    d = g(seed=1, first_sample=0, seed_dev=[9, 10])                        # seed_dev overrides both scalar fields
    assert torch.equal(d[0], x) and torch.equal(d[1], R)
    # at dt-independent scale (power 0, uniform grid) the steps differ only through the counter: unit-variance normals times sqrt(dt)
    z = x / math.sqrt(float(CO.make_grid(NS)[2] - CO.make_grid(NS)[1]))
    assert abs(float(z.mean())) < 5 / math.sqrt(z.numel()) and abs(float(z.var()) - 1) < 5 * math.sqrt(2 / z.numel())


# ==== FlowModel.sample ==================================================================================================================
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
def test_tempered_sample_vs_oracle_replay_second_set_and_no_leak(model, seeded_sd, shape):
    NS = CC.NS_E2E
    batch = CC.e2e_batch(shape)
    B, L = batch["aa"].shape
    db = _dev(batch)
    gen = batch["generate_mask"]
    plain_noise = synth.make_noise(B, L, NS, seed=5)
    before = model.sample(db, num_steps=NS, noise=plain_noise)
    for which, seed in (("a", 51), ("b", 52)):                 # 'b' runs on the sampler 'a' built: a scalar temperature, other sigmas, t_off
        c = TC.e2e_config(seeded_sd, shape, which, seed)
        traj = model.sample(db, num_steps=NS, noise=c["noise"], temper=c["temper"])
        _compare_traj(traj, c["ref"], 0, B, NS, f"{shape} temper {which}")
        eager = model.sample(db, num_steps=NS, noise=c["noise"], temper=c["temper"], use_graph=False)
        _same_traj(traj, eager, f"temper {which}: graph replay vs eager")
        plain = model.sample(db, num_steps=NS, noise=c["noise"])
        assert any(not torch.equal(plain[i]["seqs"][gen], traj[i]["seqs"][gen]) for i in range(NS)), "the temperature must change a draw"
        assert not torch.equal(plain[1]["trans"][gen], traj[1]["trans"][gen]), "the noise must change the run"
        assert all(torch.equal(plain[i]["trans"][~gen], traj[i]["trans"][~gen]) for i in range(NS))
    with pytest.raises(ValueError, match="gauss"):             # supplied categorical draws and a sigma: the normals must be supplied too
        model.sample(db, num_steps=NS, noise=plain_noise, temper={"sigma_trans": 1.0})
    _same_traj(before, model.sample(db, num_steps=NS, noise=plain_noise), "default call after tempered calls")


def test_temper_combines_with_the_conditioned_and_guided_call(model):
    """a partial start, per-residue switches, allowed classes and a guide together with a temper: graph equals eager, rows whose backbone
    switch is off keep the context's rotation and translation, every drawn type stays in its allowed set"""
    NS = CC.NS_E2E
    batch = CC.e2e_batch("L24")
    B, L = batch["aa"].shape
    db = _dev(batch)
    g = torch.Generator().manual_seed(3)
    flags, allowed = CC._mixed_flags(B, L, g), CC._allowed("random", B, L, g)
    kw = CC.sample_kwargs({"flags": flags, "aa_allowed": allowed, "t_start": 0.4, "start": "native"})
    noise = synth.make_noise(B, L, NS, seed=12)
    noise["gauss"] = TC.gauss_of(B, L, NS, 77)
    guide = GC.e2e_guide("L24", "a")
    temper = TC.e2e_temper("L24", "a")
    a = model.sample(db, num_steps=NS, noise=noise, guide=guide, temper=temper, **kw)
    _same_traj(a, model.sample(db, num_steps=NS, noise=noise, guide=guide, temper=temper, use_graph=False, **kw), "graph vs eager")
    plain = model.sample(db, num_steps=NS, noise=noise, guide=guide, **kw)
    gen = batch["generate_mask"]
    moving = gen & flags[0]
    assert (gen & ~flags[0]).any() and moving.any()
    assert not torch.equal(plain[1]["trans"][moving], a[1]["trans"][moving]) and not torch.equal(plain[1]["rotmats"][moving], a[1]["rotmats"][moving])
    rows = gen & flags[2]
    for t in a:
        assert torch.equal(t["rotmats"][~moving], t["rotmats_1"][~moving]) and torch.equal(t["trans"][~moving], t["trans_1"][~moving])
        assert allowed[rows].gather(-1, t["seqs"][rows][:, None]).all()


def test_one_sample_shards_equal_the_whole_batch(model):
    """Philox draws and seeded noise (noise = None, explicit seed): shards of one sample each with first_sample = lo and shard_temper
    reproduce the whole batch bit for bit"""
    NS = CC.NS_E2E
    batch = CC.e2e_batch("L64")
    B, L = batch["aa"].shape
    db = _dev(batch)
    temper = TC.e2e_temper("L64", "a")                        # a temperature plane [B, L]
    whole = model.sample(db, num_steps=NS, seed=9, temper=temper)
    plain = model.sample(db, num_steps=NS, seed=9)
    gen = batch["generate_mask"]
    assert not torch.equal(plain[1]["trans"][gen], whole[1]["trans"][gen])
    assert not torch.equal(whole[1]["trans"], model.sample(db, num_steps=NS, seed=10, temper=temper)[1]["trans"])
    for lo in range(B):
        sub = {k: v[lo:lo + 1].contiguous() for k, v in db.items()}
        part = model.sample(sub, num_steps=NS, seed=9, first_sample=lo, temper=sampler.shard_temper(temper, lo, lo + 1, B))
        for i in range(NS):
            for k in whole[i]:
                assert torch.equal(part[i][k], whole[i][k][lo:lo + 1]), (lo, i, k)


def test_ragged_batch_through_the_length_buckets(model):
    """lengths 48, 48, 144, 144: two buckets, each with its samples' own temperatures and normals, against buckets=False; the bounds of
    tests/test_gpu_cond.py's test of the same name"""
    NS, L0, lens = 3, 144, [48, 48, 144, 144]
    items = [synth.make_pocket_batch(1, L0, 9, seed=40 + i, lengths=[n]) for i, n in enumerate(lens)]
    batch = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    B = len(lens)
    noise = synth.make_noise(B, L0, NS, seed=6)
    noise["gauss"] = TC.gauss_of(B, L0, NS, 78)
    temper = {"seq_temperature": TC.mixed_tau(B, L0, torch.Generator().manual_seed(2)), "sigma_trans": 1.0, "sigma_rot": 0.3}
    db = _dev(batch)
    one = model.sample(db, num_steps=NS, noise=noise, buckets=False, temper=temper)
    two = model.sample(db, num_steps=NS, noise=noise, temper=temper)
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
    gen = batch["generate_mask"]
    assert not torch.equal(plain[1]["trans"][gen], two[1]["trans"][gen])
