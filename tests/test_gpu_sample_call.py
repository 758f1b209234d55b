"""The shared paths of FlowModel.sample() on a real MI355X with all four extensions at once: one packed call description
(sampler.SampleCall) fitted to the padded length or to the length buckets, one set-up (DeviceSampler.begin), one tail
(FlowModel._run_bound) behind the single engine and behind the buckets.  Everything here is a copy or a replay of the same launches,
so every comparison is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import pepflowww_amd  # noqa: E402
from pepflowww_amd import buckets, synth  # noqa: E402
import steer_cases as SC  # noqa: E402
import gpu_util as G  # noqa: E402

NS = 3
PHASES = ["noise", "engine", "encode", "bind", "setup", "capture", "loop", "range_check", "d2h"]      # sample(timings=): names and order


def _model(sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(sd, strict=True)
    return m.to(G.dev()).eval()


@pytest.fixture(scope="module")
def model(seeded_sd):
    return _model(seeded_sd)


def _dev(batch):
    return {k: v.to(G.dev()) for k, v in batch.items()}


def _same_traj(a, b, what):
    assert len(a) == len(b) == NS
    for i, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert torch.equal(x[k], y[k]), (what, i, k)


def _same_records(a, b, what):
    assert a is not None and b is not None and list(a) == list(b), what
    for k in a:
        if torch.is_tensor(a[k]):
            assert np.array_equal(a[k].numpy(), b[k].numpy(), equal_nan=True), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def _single_engine_call(expo, L0=24):
    """steer_cases.e2e_batch(): B = 4 particles of one complex at 24 residues, which the call pads to 32 -- SampleCall.fit runs for the four
    extensions; L0 = 40: the same batch padded the way PaddingCollate pads it, which the call pads to 48.  Without `expo` the categorical
    draws are the kernel's own (seed): a supplied `expo` tensor is a new device pointer in every call and part of the launch key, gauss
    and resample_u land in buffers the sampler owns."""
    batch, guide = SC.e2e_batch(), SC.e2e_guide()
    B, L = batch["aa"].shape
    if L0 != L:
        batch = buckets.sub_batch(batch, list(range(B)), L, L0)
        guide["hotspots"] = torch.cat([guide["hotspots"], torch.zeros(L0 - L, dtype=torch.bool)])
    assert batch["aa"].shape == (B, L0) and L0 % 16 != 0
    noise = synth.make_noise(B, L0, NS, seed=81)
    if not expo:
        del noise["expo"]
    noise["gauss"] = torch.randn(NS - 1, B, L0, 6, generator=torch.Generator().manual_seed(82))
    noise["resample_u"] = torch.tensor([[0.37], [0.52], [0.5]], dtype=torch.float64)
    plane = batch["generate_mask"].bool().clone()
    plane[:, ::3] = False
    kw = dict(num_steps=NS, noise=noise, seed=9, sample_seq=plane, buckets=False, guide=guide, temper=dict(SC.E2E_TEMPER),
              steer={"lam": 0.5, "ess_frac": 1.0})
    return _dev(batch), kw


@pytest.mark.parametrize("L0", [24, 40])
def test_single_engine_graph_eager_cached_sampler_and_fresh_model(model, seeded_sd, L0):
    db, kw = _single_engine_call(expo=False, L0=L0)
    smp = model.sample(db, return_sampler=True, **kw)
    graphs = (smp.graph, smp.graph_k)
    traj, rec, st = smp.trajectory(), model.last_guidance, model.last_steering
    assert graphs[0] is not None and graphs[1] is not None and smp.eng.L == L0 + 8 and smp.L_out == L0 and traj[0]["trans"].shape == (4, L0, 3)
    assert model.last_buckets is None and st["code"][:-1, 0].tolist() == [2] * (NS - 1), "ess_frac = 1: every moment resamples"
    eager = model.sample(db, use_graph=False, **kw)
    _same_traj(traj, eager, "graph replay vs eager")
    _same_records(rec, model.last_guidance, "guidance record, graph vs eager")
    _same_records(st, model.last_steering, "steering record, graph vs eager")
    # other parameter values on the cached sampler: nothing is captured again
    plane = ~kw["sample_seq"] & db["generate_mask"].bool().cpu()
    other = {**kw, "sample_seq": plane, "guide": {**kw["guide"], "scale": 0.02, "power": 2}, "temper": {"seq_temperature": 1.3, "sigma_trans": 0.5},
             "steer": {"lam": 0.3, "every": 2, "ess_frac": 0.9, "groups": torch.tensor([3, 1, 3, 1])}, "seed": 11}
    other["noise"] = {**kw["noise"], "resample_u": torch.tensor([[0.1, 0.9], [0.6, 0.2], [0.5, 0.5]], dtype=torch.float64)}
    smp2 = model.sample(db, return_sampler=True, **other)
    assert smp2 is smp and smp.graph is graphs[0] and smp.graph_k is graphs[1], "the second call re-captures nothing"
    got, rec2, st2 = smp2.trajectory(), model.last_guidance, model.last_steering
    assert st2["groups"].tolist() == [0, 1, 0, 1] and st2["ess"].shape == (NS, 2)
    fresh = _model(seeded_sd)
    _same_traj(got, fresh.sample(db, **other), "second parameter set on the cached sampler vs a fresh model")
    _same_records(rec2, fresh.last_guidance, "guidance record, cached sampler vs fresh model")
    _same_records(st2, fresh.last_steering, "steering record, cached sampler vs fresh model")


def test_single_engine_timings_name_every_phase(model):
    db, kw = _single_engine_call(expo=True)
    tm = {}
    traj = model.sample(db, timings=tm, **kw)
    assert list(tm) == PHASES and all(v >= 0 for v in tm.values()), tm
    assert len(traj) == NS and model.last_buckets is None and model.last_steering is not None


def test_buckets_timings_last_buckets_and_returned_sampler(model):
    """the ragged two-group batch of test_gpu_steer.test_ragged_batch_two_groups_through_the_length_buckets: 48, 144, 48, 144 residues"""
    L0, B = 144, 4
    items = [synth.make_pocket_batch(1, L0, 9, seed=40 + i, lengths=[n]) for i, n in ((0, 48), (1, 144))]
    batch = {k: torch.cat([items[0][k], items[1][k], items[0][k], items[1][k]], 0) for k in items[0]}
    noise = synth.make_noise(B, L0, NS, seed=6)
    noise["gauss"] = torch.randn(NS - 1, B, L0, 6, generator=torch.Generator().manual_seed(79))
    noise["resample_u"] = torch.tensor([[0.37, 0.61], [0.52, 0.44], [0.5, 0.5]], dtype=torch.float64)
    kw = dict(num_steps=NS, noise=noise, guide={"weights": [1.0, 1.0, 1.0, 0.0], "scale": 0.05}, temper={"sigma_trans": 1.0, "sigma_rot": 0.3},
              steer={"groups": torch.tensor([7, 2, 7, 2]), "lam": 0.2, "ess_frac": 1.0})
    db = _dev(batch)
    tm = {}
    traj = model.sample(db, timings=tm, **kw)
    assert list(tm) == PHASES and all(v >= 0 for v in tm.values()), tm
    assert model.last_buckets == [(2, 48), (2, 144)], model.last_buckets
    rec, st = model.last_guidance, model.last_steering
    assert st["groups"].tolist() == [0, 1, 0, 1] and rec["energy"].shape[:2] == (NS, B)
    smp = model.sample(db, return_sampler=True, **kw)
    assert type(smp).__name__ == "BucketedSampler" and [(s.eng.B, s.eng.L) for s in smp.samplers] == model.last_buckets
    _same_traj(smp.trajectory(), traj, "returned bucketed sampler vs the first call's trajectory")
    _same_records(rec, model.last_guidance, "guidance record of the repeated bucketed call")
    _same_records(st, model.last_steering, "steering record of the repeated bucketed call")
