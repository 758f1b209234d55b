"""Steered sampling on a real MI355X: pf_sampler_steer alone (stand-alone mode through the C ABI and geometry.resample_particles), behind
pf_guidance_fwd -> pf_sampler_temper -> pf_sampler_step_cond on fabricated "network outputs", and end to end through
FlowModel.sample(steer=...).

Tolerances.  The decide kernel and tests/steer_oracle.py compute in double in the same order, so only exp() can differ in its last
bits: ancestors and codes EXACT, ESS and log-weights to 1e-12 relative -- on cases whose every decision has a margin >= 1e-9
(tests/steer_cases.py; asserted on the CPU in tests/test_steer_cpu.py).  The gather is a copy: bit-equal.  End to end: the oracle's
decide step fed the device's own recorded fp32 energies must reproduce the device's record exactly; the recorded energies are held to
the rule of tests/test_gpu_guide.py, the trajectory to test_gpu_bigshape._compare_traj against the oracle replay with the device's
ancestor record forced, and the oracle's FREE decisions equal the device's because the case's margins exceed what that energy tolerance
can move a weight by (steer_cases.weight_shift_bound; asserted on the CPU)."""
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
import steer_cases as SC  # noqa: E402
import steer_oracle as SO  # noqa: E402
import gpu_util as G  # noqa: E402
from test_gpu_bigshape import _compare_traj  # noqa: E402
from test_gpu_cond import STATE, TRAJ, Abi, cu  # noqa: E402
from test_gpu_guide import Guidance, _energy_tolerance  # noqa: E402
from test_gpu_temper import Temper  # noqa: E402

RTOL = 1e-12
CANARY = -7


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
    assert np.all(err <= RTOL), (what, float(err.max()))


class Steer:
    """device buffers of one pf_sampler_steer_args; groups from labels, canary-filled records"""

    def __init__(self, B, L, NS, labels, params, energy, u=None, step=None, ts=None, state=None, seed=0, first_sample=0, ids=None, logw=None):
        dev = G.dev()
        ptr, members, self.group_of, self.G = sampler.pack_groups(np.asarray(labels))
        f8 = torch.float64
        self.t = {"params": torch.tensor(list(params) + [0.0] * (8 - len(params)), dtype=f8, device=dev), "group_ptr": cu(torch.from_numpy(ptr)),
                  "members": cu(torch.from_numpy(members)), "n_groups": torch.tensor([self.G], dtype=torch.int32, device=dev),
                  "energy": energy, "logw": torch.zeros(B, dtype=f8, device=dev) if logw is None else cu(logw.to(f8)),
                  "eprev": torch.zeros(B, dtype=f8, device=dev),
                  "ancestors": torch.full((NS, B), CANARY, dtype=torch.int32, device=dev), "logw_rec": torch.full((NS, B), float(CANARY), dtype=f8, device=dev),
                  "ess": torch.full((NS, B), float(CANARY), dtype=f8, device=dev), "code": torch.full((NS, B), CANARY, dtype=torch.int32, device=dev)}
        if u is not None:
            self.t["u"] = cu(torch.as_tensor(u, dtype=f8))
        if step is not None:
            self.t["step"], self.t["ts"] = step, ts
        if ids is not None:
            self.t["sample_ids"] = cu(torch.as_tensor(ids, dtype=torch.int64))
        a = self.args = _capi.SamplerSteerArgs()
        for k, v in self.t.items():
            setattr(a, k, v.data_ptr())
        for k, v in (state or {}).items():
            setattr(a, k, v.data_ptr())
        a.seed, a.first_sample, a.B, a.L, a.num_steps, a.max_group = seed, first_sample, B, L, NS, int(np.diff(ptr[:self.G + 1]).max())

    def launch(self):
        _capi.check(_capi.load().pf_sampler_steer(C.byref(self.args), _capi.stream_ptr()), "pf_sampler_steer")

    def rec(self):
        out = {k: self.t[k].cpu().numpy() for k in ("ancestors", "logw_rec", "ess", "code", "logw", "eprev")}
        return out


# ==== 1: the stand-alone kernel against the oracle ======================================================================================
@pytest.mark.parametrize("kind, ukind, ess_frac", SC.STANDALONE)
def test_standalone_decision_vs_oracle(kind, ukind, ess_frac):
    case = SC.standalone_case(kind, ukind, ess_frac)
    ref = SC.standalone_ref(case)
    B, Gn = case["B"], len(case["groups"])
    h = Steer(B, 1, 1, case["labels"].numpy(), [case["lam"], 1, ess_frac, 0.0, 1.0], cu(case["energy"]), u=case["u"], logw=case["logw"])
    h.launch()
    got = h.rec()
    assert np.array_equal(got["ancestors"][0], ref["ancestors"]), f"{kind} {ukind}: ancestors differ"
    assert got["code"][0, :Gn].tolist() == list(ref["code"]) and (got["code"][0, Gn:] == CANARY).all()
    _close(got["ess"][0, :Gn], ref["ess"], "ess")
    assert (got["ess"][0, Gn:] == CANARY).all(), "workgroups beyond n_groups return"
    _close(got["logw_rec"][0], ref["logw_rec"], "logw before the reset")
    _close(got["logw"], ref["logw"], "logw after the reset")
    again = Steer(B, 1, 1, case["labels"].numpy(), [case["lam"], 1, ess_frac, 0.0, 1.0], cu(case["energy"]), u=case["u"], logw=case["logw"])
    again.launch()
    for k, v in again.rec().items():
        assert np.array_equal(v, got[k], equal_nan=True), (k, "two runs, the same bits")
    print(f"{kind} {ukind} {ess_frac}: codes {sorted(set(ref['code']))}, moved {int((ref['ancestors'] != np.arange(B)).sum())} of {B}, "
          f"smallest margin {min(ref['margin_c']):.2e}")


def test_resample_particles_gathers_in_place_and_checks_its_arguments():
    case = SC.standalone_case("random", "mid")
    B, L = case["B"], 3
    logw = torch.from_numpy(SC.standalone_ref(case)["logw_rec"])                     # the weights the decision above was taken on
    ref = SC.standalone_ref({**case, "logw": logw, "energy": torch.zeros(B, 5), "lam": 0.0})
    g = torch.Generator().manual_seed(1)
    state = [cu(torch.randn(B, L, w, generator=g)) for w in (9, 3, 5)] + [cu(torch.randint(0, 20, (B, L), generator=g))] + \
            [cu(torch.randn(B, L, w, generator=g)) for w in (20, 3, 20)]
    before = [v.cpu().clone() for v in state]
    out = geometry.resample_particles(cu(logw), case["labels"], u=torch.from_numpy(case["u"]), state=state)
    anc = out["ancestors"].cpu()
    assert np.array_equal(anc.numpy(), ref["ancestors"]) and (anc != torch.arange(B)).any() and out["code"].tolist() == [2] * len(case["groups"])
    for v, b in zip(state, before):
        assert torch.equal(v.cpu(), b[anc]), "every slot holds its ancestor's rows, bit for bit"
    assert float(out["logw"].abs().max()) == 0
    keep = geometry.resample_particles(cu(logw), case["labels"], u=torch.from_numpy(case["u"]), ess_frac=0.0)
    assert torch.equal(keep["ancestors"].cpu(), torch.arange(B)) and keep["code"].tolist() == [1] * len(case["groups"])
    assert torch.equal(keep["logw"].cpu(), logw)
    a, b = (geometry.resample_particles(cu(logw), case["labels"], seed=s)["ancestors"] for s in (3, 3))
    assert torch.equal(a, b) and not torch.equal(a, geometry.resample_particles(cu(logw), case["labels"], seed=4)["ancestors"])
    with pytest.raises(ValueError, match="at most 1024"):
        geometry.resample_particles(cu(torch.zeros(1025, dtype=torch.float64)))
    with pytest.raises(ValueError, match="ess_frac"):
        geometry.resample_particles(cu(logw), ess_frac=1.5)
    with pytest.raises(ValueError, match="one per group"):
        geometry.resample_particles(cu(logw), case["labels"], u=torch.tensor([0.5]))
    with pytest.raises(_capi.PepflowHipError):
        geometry.resample_particles(logw, case["labels"])                         # a CPU tensor: no fallback


# ==== 2, 3: guidance -> temper -> step -> steer on fabricated predictions ===============================================================
def _chain(shape):
    """-> per step: state before the steer entry, after it, the device records; plus the harnesses"""
    case = SC.chain_case(shape)
    B, L, NS = case["B"], case["L"], case["NS"]
    rows, dev = B * L, G.dev()
    grid = CO.make_grid(NS)
    h = Abi(case, case["noise"], grid)
    cond = h.cond(flags=case["flags"])
    gd = Guidance(case, SC.CHAIN_GUIDE)
    raw = torch.zeros(rows, 3, device=dev)
    ga = gd.args
    ga.pred_trans, ga.guided_trans = raw.data_ptr(), h.t["pred_trans"].data_ptr()
    ga.res_flags, ga.step, ga.ts = cond.res_flags, h.t["step"].data_ptr(), h.t["ts"].data_ptr()
    tp = Temper(h, SC.CHAIN_TEMPER, cond, case["gauss"])
    assert tp.tau is None
    tp.raw = h.t["pred_logits"]                                # no temperature plane: the step kernel reads the logits themselves
    p = SC.CHAIN_STEER
    st = Steer(B, L, NS, case["labels"].numpy(), [p["lam"], p["every"], p["ess_frac"], 0.0, 1.0], gd.t["energy"], u=_pad_u(case["u"], B),
               step=h.t["step"], ts=h.t["ts"], state={k: h.t[k] for k in STATE})
    lib, s0, nz = _capi.load(), _capi.stream_ptr(), h.noise
    _capi.check(lib.pf_sampler_init_cond(C.byref(h.args), C.byref(cond), nz["rot0"].data_ptr(), nz["trans0"].data_ptr(), nz["ang0"].data_ptr(),
                                         nz["simplex0"].data_ptr(), s0), "pf_sampler_init_cond")
    snap = lambda keys: {k: h.t[k].cpu().clone() for k in keys}  # noqa: E731
    other = TRAJ + ("pred_rot", "pred_trans", "pred_ang_raw", "pred_logits", "rot1", "trans1", "ang1", "seq1", "gen_mask", "res_mask", "step", "ts", "t_out")
    pre, post, untouched = [], [], True
    for s in range(NS + 2):                                    # two extra steps past the end
        if s < NS:
            for buf, v in zip((h.t["pred_rot"], raw, h.t["pred_ang_raw"], h.t["pred_logits"]), case["preds"][s]):
                buf.copy_(v.reshape(buf.shape))
        _capi.check(lib.pf_guidance_fwd(C.byref(ga), s0), "pf_guidance_fwd")
        tp.launch()
        _capi.check(lib.pf_sampler_step_cond(C.byref(h.args), C.byref(cond), s0), "pf_sampler_step_cond")
        before, rest, recs = snap(STATE), snap(other), st.rec()
        energy = gd.t["energy"].cpu().clone()
        st.launch()
        after, rest2 = snap(STATE), snap(other)
        untouched = untouched and all(torch.equal(rest[k], rest2[k]) for k in other) and torch.equal(energy, gd.t["energy"].cpu())
        if s < NS:
            pre.append(before)
            post.append(after)
        else:                                                  # past the end: nothing at all is written
            assert all(torch.equal(before[k], after[k]) for k in STATE), s
            assert all(np.array_equal(v, st.rec()[k], equal_nan=True) for k, v in recs.items()), s
    assert untouched, "trajectory, predictions, context, step counter and the guidance record keep their bits"
    return case, pre, post, st, gd


def _pad_u(u, B):
    out = torch.full((u.shape[0], B), 0.5, dtype=torch.float64)
    out[:, :u.shape[1]] = u
    return out


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_chain_gathers_ancestors_records_match_and_nothing_else_is_written(shape):
    case, pre, post, st, gd = _chain(shape)
    B, L, NS = case["B"], case["L"], case["NS"]
    got = st.rec()
    groups = SO.groups_of(case["labels"].numpy(), B)
    Gn = len(groups)
    energy = gd.t["energy"].cpu().numpy()
    grid = CO.make_grid(NS)
    logw, eprev = np.zeros(B), np.zeros(B)
    p = SO.params(SC.CHAIN_STEER)
    moved = 0
    for s in range(NS):
        ref = SO.step_all(energy[s], logw, eprev, groups, p, s, NS, grid[s], case["u"][s].numpy())
        assert min(ref["margin_c"]) >= SC.MARGIN, (s, ref["margin_c"])
        anc = got["ancestors"][s]
        assert np.array_equal(anc, ref["ancestors"]), (s, anc, ref["ancestors"])
        assert got["code"][s, :Gn].tolist() == list(ref["code"]) and (got["code"][s, Gn:] == CANARY).all(), (s, got["code"][s])
        _close(got["ess"][s, :Gn], ref["ess"], f"step {s} ess")
        _close(got["logw_rec"][s], ref["logw_rec"], f"step {s} logw")
        assert (got["ess"][s, Gn:] == CANARY).all()
        ix = torch.as_tensor(anc, dtype=torch.int64)
        for k in STATE:                                        # slot b holds the pre-gather state of its ancestor, bit for bit
            w = pre[s][k].reshape(B, L, -1)
            assert torch.equal(post[s][k].reshape(B, L, -1), w[ix]), (s, k)
            keep = torch.as_tensor(anc == np.arange(B))
            assert torch.equal(post[s][k].reshape(B, L, -1)[keep], w[keep]), (s, k, "rows of slots that were no destination")
        moved += int((anc != np.arange(B)).sum())
        if s == NS - 1:
            assert (anc == np.arange(B)).all() and set(ref["code"]) == {0}, "the last step never gathers"
    _close(got["logw"], logw, "final logw")
    _close(got["eprev"], eprev, "final eprev")
    assert moved > 0, "a chain that never moves a particle shows nothing"
    print(f"{shape}: {moved} slots moved; codes {got['code'][:, :Gn].tolist()}")


# ==== 4: the in-kernel uniform ==========================================================================================================
def _decide_with_own_u(B, NS, s, labels, logw, seed, first_sample=0, ids=None):
    dev = G.dev()
    step = torch.tensor([s + 1, 0], dtype=torch.int32, device=dev)
    ts = cu(CO.make_grid(NS))
    h = Steer(B, 1, NS, labels, [0.0, 1, 1.0, 0.0, 1.0], torch.zeros(NS, B, 5, device=dev), step=step, ts=ts, seed=seed,
              first_sample=first_sample, ids=ids, logw=logw)
    h.launch()
    got = h.rec()
    assert (got["ancestors"][[i for i in range(NS) if i != s]] == CANARY).all(), "only slot s is written"
    return got["ancestors"][s]


def test_in_kernel_uniform_vs_the_integer_restatement_and_shards():
    B, NS = 192, 5
    g = torch.Generator().manual_seed(8)
    labels = np.repeat([5, 1, 9], 64)[torch.randperm(B, generator=g).numpy()]
    labels[:64] = np.sort(labels[:64])                         # (any labels: the groups stay interleaved)
    logw = 1.5 * torch.randn(B, generator=g, dtype=torch.float64)
    groups = SO.groups_of(labels, B)
    seed = (5 << 32) | 17
    ids = np.array([(1 << 32) + 3 * b for b in range(B)])

    def ref(s, seed, ids):
        out = np.arange(B)
        for m in groups:
            d = SO.decide(np.zeros((len(m), 5), np.float32), logw.numpy()[m], np.zeros(len(m)), 0.0, 1.0, True, True, SO.philox_u(seed, s, ids[m[0]]))
            assert d["margin_c"] >= SC.MARGIN
            out[m] = m[d["anc"]]
        return out
    a = _decide_with_own_u(B, NS, 1, labels, logw, seed, ids=ids)
    assert np.array_equal(a, ref(1, seed, ids)) and (a != np.arange(B)).any()
    for other in (_decide_with_own_u(B, NS, 2, labels, logw, seed, ids=ids), _decide_with_own_u(B, NS, 1, labels, logw, seed + 1, ids=ids),
                  _decide_with_own_u(B, NS, 1, labels, logw, seed, ids=ids + 1)):
        assert not np.array_equal(other, a), "keyed by step, seed and the first member's global sample id"
    assert np.array_equal(_decide_with_own_u(B, NS, 2, labels, logw, seed, ids=ids), ref(2, seed, ids))
    f = _decide_with_own_u(B, NS, 1, labels, logw, seed, first_sample=40)      # sample_ids = NULL: first_sample + m_0
    assert np.array_equal(f, ref(1, seed, np.arange(B) + 40))
    # a run of whole groups as a shard draws what the whole batch draws
    lab2 = np.repeat([0, 1, 2], 64)
    whole = _decide_with_own_u(B, NS, 1, lab2, logw, seed, first_sample=0)
    part = _decide_with_own_u(128, NS, 1, lab2[64:], logw[64:], seed, first_sample=64)
    assert np.array_equal(part + 64, whole[64:])
    assert _decide_with_own_u(B, NS, NS - 1, labels, logw, seed, ids=ids).tolist() == list(range(B)), "the last step is no moment"


# ==== 5 - 9: FlowModel.sample ===========================================================================================================
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


def _replay_decisions(rec, steer, grid, u, B):
    """the oracle's decide step fed the device's own recorded fp32 energies -> its records, step by step"""
    groups = SO.groups_of(SO.params(steer)["groups"], B)
    logw, eprev = np.zeros(B), np.zeros(B)
    NS = rec.shape[0]
    return [SO.step_all(rec[s].numpy(), logw, eprev, groups, SO.params(steer), s, NS, grid[s], np.asarray(u[s])) for s in range(NS)], logw


def _check_records(st, refs, what):
    Gn = st["ess"].shape[1]
    for s, ref in enumerate(refs):
        assert np.array_equal(st["ancestors"][s].numpy(), ref["ancestors"]), (what, s, st["ancestors"][s], ref["ancestors"])
        assert st["code"][s].tolist() == list(ref["code"]), (what, s)
        _close(st["ess"][s].numpy(), ref["ess"], f"{what} step {s} ess")
        _close(st["logw"][s].numpy(), ref["logw_rec"], f"{what} step {s} logw")
    assert Gn == len(refs[0]["ess"])


def test_steered_sample_vs_oracle(model, seeded_sd):
    NS, B = CC.NS_E2E, SC.E2E_B
    c = SC.e2e_case(seeded_sd)
    db = _dev(c["batch"])
    grid = CO.make_grid(NS)
    traj = model.sample(db, num_steps=NS, noise=c["noise"], guide=c["guide"], temper=c["temper"], steer=c["steer"])
    st, rec = model.last_steering, model.last_guidance
    assert st["ancestors"].shape == (NS, B) and st["ess"].shape == (NS, 1) and st["weights"].shape == (B,) and not st["logw"].is_cuda
    # (a) the decide step on the device's own energies
    refs, logw = _replay_decisions(rec["energy"], c["steer"], grid, c["noise"]["resample_u"], B)
    _check_records(st, refs, "e2e")
    w = np.exp(logw - logw.max())
    _close(st["weights"].numpy(), w / np.cumsum(w)[-1], "weights")
    # (b) the recorded energies against the oracle's, under the rule of tests/test_gpu_guide.py
    tol = _energy_tolerance(c["batch"], c["guide"], c["energy"], c["xs"])
    d = (rec["energy"].double() - c["energy"]).abs()
    print(f"worst energy deviation / tolerance = {float((d / tol).max()):.3f}")
    assert (d <= tol).all(), float((d / tol).max())
    # (c) the trajectory against the oracle replay with the device's ancestor record forced
    with torch.no_grad():
        forced = SO.sample(seeded_sd, c["batch"], c["noise"], NS, guide=c["guide"], temper=c["temper"], steer=c["steer"], encoded=c["encoded"],
                           force=st["ancestors"].numpy())
    _compare_traj(traj, forced, 0, B, NS, "steered, ancestors forced")
    # (d) the oracle's free decisions equal the device's (the case's margins: tests/test_steer_cpu.py)
    assert np.array_equal(st["ancestors"].numpy(), c["srec"]["ancestors"]) and st["code"].numpy().tolist() == c["srec"]["code"].tolist()
    assert (st["ancestors"][0] != torch.arange(B)).any()
    _compare_traj(traj, c["ref"], 0, B, NS, "steered, free")
    eager = model.sample(db, num_steps=NS, noise=c["noise"], guide=c["guide"], temper=c["temper"], steer=c["steer"], use_graph=False)
    _same_traj(traj, eager, "graph replay vs eager")
    assert torch.equal(model.last_steering["ancestors"], st["ancestors"]) and torch.equal(model.last_steering["logw"], st["logw"])
    lin = sampler.steer_lineage(st["ancestors"])
    assert torch.equal(lin[-1], torch.arange(B)) and np.array_equal(lin.numpy(), SO.lineage_brute(st["ancestors"].numpy()))
    with pytest.raises(ValueError, match="resample_u"):        # supplied categorical draws: the uniforms must be supplied too
        model.sample(db, num_steps=NS, noise={k: v for k, v in c["noise"].items() if k != "resample_u"}, guide=c["guide"], temper=c["temper"], steer=c["steer"])
    with pytest.raises(ValueError, match="steer needs guide"):
        model.sample(db, num_steps=NS, noise=c["noise"], temper=c["temper"], steer=c["steer"])


def test_ess_frac_zero_is_the_unsteered_trajectory_and_weights_accumulate(model):
    NS, B = CC.NS_E2E, SC.E2E_B
    db = _dev(SC.e2e_batch())
    guide, temper, noise = SC.e2e_guide(), dict(SC.E2E_TEMPER), SC.e2e_noise(62)
    plain_noise = {k: v for k, v in noise.items() if k != "resample_u"}
    plain = model.sample(db, num_steps=NS, noise=plain_noise, guide=guide, temper=temper)
    steer = {"lam": 0.05, "ess_frac": 0.0, "t_on": 0.2}
    got = model.sample(db, num_steps=NS, noise=noise, guide=guide, temper=temper, steer=steer)
    _same_traj(plain, got, "ess_frac = 0")
    st = model.last_steering
    refs, logw = _replay_decisions(model.last_guidance["energy"], steer, CO.make_grid(NS), noise["resample_u"], B)
    _check_records(st, refs, "ess_frac = 0")
    assert st["code"][:, 0].tolist() == [0, 1, 1, 0], "t = 0.01 lies before t_on; the last step is no moment"
    assert float(st["logw"][0].abs().max()) == 0 and float(st["logw"][-1].abs().min()) > 0
    assert torch.equal(st["ancestors"], torch.arange(B).expand(NS, B))


def test_a_copy_continues_as_its_ancestor_would(model):
    """sigmas 0, the categorical draws equal inside the group, a resampling forced at every step: from the step after a copy, the copy's
    recorded predictions are its ancestor slot's, bit for bit -- the engine holds no per-slot state besides the seven gathered tensors"""
    NS, B = CC.NS_E2E, SC.E2E_B
    db = _dev(SC.e2e_batch())
    noise = SC.e2e_noise(63, equal_expo=True)
    del noise["gauss"]
    traj = model.sample(db, num_steps=NS, noise=noise, guide=SC.e2e_guide(), temper={"seq_temperature": 0.7},
                        steer={"lam": 0.5, "ess_frac": 1.0})
    anc = model.last_steering["ancestors"]
    assert model.last_steering["code"][:-1, 0].tolist() == [2] * (NS - 1)
    assert (anc[0] != torch.arange(B)).any(), "the first resampling must copy a particle"
    checked = 0
    for s in range(NS - 1):
        for b in range(B):
            a = int(anc[s, b])
            if a != b:
                checked += 1
                for k in ("rotmats", "trans", "angles", "seqs", "seqs_simplex"):
                    assert torch.equal(traj[s + 1][k][b], traj[s + 1][k][a]), (s, b, a, k)
    assert not torch.equal(traj[0]["trans"][0], traj[0]["trans"][1]), "the particles start apart"
    print(f"{checked} copies followed")


def test_cached_sampler_serves_other_parameters_and_unsteered_calls_stay(model, seeded_sd):
    """in-kernel draws throughout (noise = None, an explicit seed): a supplied `expo` tensor is a new device pointer in every call and
    part of the launch key, whatever the call steers by"""
    NS, B = CC.NS_E2E, SC.E2E_B
    db = _dev(SC.e2e_batch())
    guide, temper = SC.e2e_guide(), dict(SC.E2E_TEMPER)
    before = model.sample(db, num_steps=NS, seed=9, guide=guide, temper=temper)
    smp = model.sample(db, num_steps=NS, seed=9, guide=guide, temper=temper, steer={"lam": 0.05, "ess_frac": 1.0}, return_sampler=True)
    graphs = (smp.graph, smp.graph_k)
    first = model.last_steering
    assert graphs[0] is not None and (first["ancestors"][:-1] != torch.arange(B)).any()
    other = {"lam": 0.3, "every": 2, "ess_frac": 0.9, "groups": torch.tensor([3, 1, 3, 1])}
    smp2 = model.sample(db, num_steps=NS, seed=9, guide=guide, temper=temper, steer=other, return_sampler=True)
    assert smp2 is smp and smp.graph is graphs[0] and smp.graph_k is graphs[1], "the second call re-captures nothing"
    got, st = smp2.trajectory(), model.last_steering
    assert st["groups"].tolist() == [0, 1, 0, 1] and st["ess"].shape == (NS, 2)
    fresh = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    fresh.load_state_dict(seeded_sd, strict=True)
    fresh = fresh.to(G.dev()).eval()
    want = fresh.sample(db, num_steps=NS, seed=9, guide=guide, temper=temper, steer=other)
    _same_traj(got, want, "second parameter set on the cached sampler vs a fresh model")
    for k in ("ancestors", "logw", "ess", "code", "weights"):
        assert np.array_equal(st[k].numpy(), fresh.last_steering[k].numpy(), equal_nan=True), k
    assert st["code"][0].tolist() == [0, 0] and (st["code"][1] != 0).all(), "every = 2: step 0 is no moment, step 1 is"
    _same_traj(before, model.sample(db, num_steps=NS, seed=9, guide=guide, temper=temper), "guided + tempered call after steered calls")
    assert model.last_steering is None


def test_ragged_batch_two_groups_through_the_length_buckets(model):
    """two groups of different length (48, 48 | 144, 144) through the length buckets against each group run alone; records in caller order"""
    NS, L0 = 3, 144
    items = [synth.make_pocket_batch(1, L0, 9, seed=40 + i, lengths=[n]) for i, n in ((0, 48), (1, 144))]
    batch = {k: torch.cat([items[0][k], items[1][k], items[0][k], items[1][k]], 0) for k in items[0]}       # interleaved: 48, 144, 48, 144
    B = 4
    labels = torch.tensor([7, 2, 7, 2])
    noise = synth.make_noise(B, L0, NS, seed=6)
    noise["gauss"] = torch.randn(NS - 1, B, L0, 6, generator=torch.Generator().manual_seed(79))
    noise["resample_u"] = torch.tensor([[0.37, 0.61], [0.52, 0.44], [0.5, 0.5]], dtype=torch.float64)
    guide = {"weights": [1.0, 1.0, 1.0, 0.0], "scale": 0.05}
    temper = {"sigma_trans": 1.0, "sigma_rot": 0.3}
    steer = {"groups": labels, "lam": 0.2, "ess_frac": 1.0}
    db = _dev(batch)
    both = model.sample(db, num_steps=NS, noise=noise, guide=guide, temper=temper, steer=steer)
    assert model.last_buckets == [(2, 48), (2, 144)], model.last_buckets
    st = model.last_steering
    assert st["groups"].tolist() == [0, 1, 0, 1] and st["ancestors"].shape == (NS, B) and st["ess"].shape == (NS, 2)
    assert (st["ancestors"][:-1] != torch.arange(B)).any()
    # the decisions must not hang by a thread: the two runs agree to kernel-form precision only
    refs, _ = _replay_decisions(model.last_guidance["energy"], steer, CO.make_grid(NS), noise["resample_u"], B)
    _check_records(st, refs, "ragged")
    assert min(min(r["margin_c"]) for r in refs) > 1e-4, [r["margin_c"] for r in refs]
    ok = batch["res_mask"]
    for g, idx in enumerate(([0, 2], [1, 3])):
        sub = {k: v[idx].contiguous() for k, v in db.items()}
        nz = {k: (v[:, idx] if k in ("expo", "gauss") else v[:, g:g + 1] if k == "resample_u" else v[idx]).contiguous() for k, v in noise.items()}
        alone = model.sample(sub, num_steps=NS, noise=nz, guide=guide, temper=temper, steer={"lam": 0.2, "ess_frac": 1.0})
        sa = model.last_steering
        ix = torch.tensor(idx)
        assert torch.equal(ix[sa["ancestors"]], st["ancestors"][:, idx]), (g, sa["ancestors"], st["ancestors"])
        assert torch.equal(sa["code"][:, 0], st["code"][:, g])
        assert float((sa["ess"][:, 0] - st["ess"][:, g]).abs().max()) < 1e-3 and float((sa["logw"] - st["logw"][:, idx]).abs().max()) < 1e-3
        for i in range(NS):
            assert torch.equal(alone[i]["seqs"], both[i]["seqs"][idx]), f"group {g} step {i}: sequences differ"
            m = ok[idx]
            for k in ("rotmats", "trans"):
                e = G.rel_err(both[i][k][idx][m], alone[i][k][m])
                assert e < 3e-5 * (1 + 3 * i), (g, i, k, e)
            d = (both[i]["angles"][idx][m] - alone[i]["angles"][m]).abs()
            assert torch.minimum(d, 2 * math.pi - d).max() < 1e-4 * (1 + 3 * i), (g, i, "angles")
