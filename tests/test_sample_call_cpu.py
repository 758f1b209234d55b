"""sampler.SampleCall (one packed description of a sample() call) and DeviceSampler.begin (its one set-up path) against the module-level
functions they compose: make == make_cond, make_guide, make_temper, check_gauss, make_steer, check_resample_u in that order (the first
error of a call with two bad arguments included), fit == the four fit_* one by one, kinds == the four `is not None`, and the order of
the set-up calls on a recording stand-in.  Host code only."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from pepflowww_amd import sampler  # noqa: E402
from pepflowww_amd.sampler import DeviceSampler, SampleCall  # noqa: E402
import cond_cases as CC  # noqa: E402
import guide_cases as GC  # noqa: E402
import steer_cases as SC  # noqa: E402
import temper_cases as TC  # noqa: E402

SHAPE = "3x16"
EXTENSIONS = ("cond", "guide", "temper", "steer")


def _same(a, b, what=""):
    """equal, entry by entry: tensors by dtype, shape and value"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    else:
        assert type(a) is type(b) and a == b, (what, a, b)


def _six(batch, num_steps, flags=(True, True, True), *, t_start=None, ts=None, start=None, aa_allowed=None, guide=None, temper=None, steer=None,
         noise=None):
    """the six functions one by one, in the documented order -> the fields of a SampleCall"""
    B, L = batch["aa"].shape
    grid, fl, cond = sampler.make_cond(B, L, num_steps, *flags, t_start, ts, start, aa_allowed)
    g = sampler.make_guide(guide, B, L, batch.get("generate_mask"), batch.get("res_mask"))
    t = sampler.make_temper(temper, B, L)
    sampler.check_gauss(noise, t, int(num_steps), B, L)
    s = sampler.make_steer(steer, B, L, batch, cond, g, t)
    sampler.check_resample_u(noise, s, int(num_steps))
    return {"grid": grid, "flags": fl, "cond": cond, "guide": g, "temper": t, "steer": s}


def _check_make(batch, num_steps, flags=(True, True, True), **kw):
    want = _six(batch, num_steps, flags, **kw)
    call = SampleCall.make(batch, num_steps, *flags, **kw)
    _same(vars(call), want, "SampleCall.make")
    assert call.kinds == {k: want[k] is not None for k in EXTENSIONS}
    return call


def _abi_batch(case):
    return {**case["batch"], "aa": case["gt"][3]}


@pytest.mark.parametrize("name", sorted(CC.ABI_CONFIGS))
def test_make_packs_the_conditioning_cases(name):
    cfg = CC.abi_config(SHAPE, name)
    kw = dict(cfg["kw"])
    call = _check_make(_abi_batch(cfg["case"]), cfg["case"]["NS"], kw.pop("flags"), noise=cfg["noise"], **kw)
    assert call.kinds["cond"] == (name != "nonuniform_ts") and not (call.kinds["guide"] or call.kinds["temper"] or call.kinds["steer"])


@pytest.mark.parametrize("name", GC.CONFIGS)
def test_make_packs_the_guidance_cases(name):
    case = GC.abi_case(SHAPE)
    # ("other" puts sample 0's hot spots on every sample, whatever is generated there: a case of the kernel, packed without the masks)
    batch = _abi_batch(case) if name != "other" else {"aa": case["gt"][3]}
    call = _check_make(batch, case["NS"], case["flags"], guide=GC.abi_guide(SHAPE, name), noise=case["noise"])
    assert call.kinds == {"cond": True, "guide": True, "temper": False, "steer": False}


@pytest.mark.parametrize("name", TC.ALL_CONFIGS)
def test_make_packs_the_tempering_cases(name):
    case = TC.abi_case(SHAPE)
    temper, grid_kw = TC.abi_temper(SHAPE, name)
    noise = {**case["noise"], "gauss": TC.gauss_of(case["B"], case["L"], TC.NS, 4000)}
    call = _check_make(_abi_batch(case), TC.NS, case["flags"], temper=temper, noise=noise, **grid_kw)
    assert call.kinds["temper"] and not call.kinds["guide"]


@pytest.mark.parametrize("groups", [None, [5, 5, 2, 2]])
def test_make_packs_the_steering_case(groups):
    batch, noise = SC.e2e_batch(), SC.e2e_noise(61)
    steer = dict(SC.E2E_STEER)
    if groups is not None:
        steer["groups"] = torch.tensor(groups)
        noise["resample_u"] = noise["resample_u"].repeat(1, 2).contiguous()
    plane = torch.zeros(batch["aa"].shape, dtype=torch.bool)
    plane[:, ::2] = True
    call = _check_make(batch, CC.NS_E2E, (True, True, plane), t_start=0.3, start="native", guide=SC.e2e_guide(), temper=dict(SC.E2E_TEMPER),
                       steer=steer, noise=noise)
    assert all(call.kinds.values()) and call.steer["n_groups"] == (1 if groups is None else 2)


TWO_ERRORS = {
    "t_start, then temper": dict(t_start=1.5, temper={"bogus": 1}),
    "guide, then steer": dict(guide={"power": 7}, steer={"lam": -1.0}),
    "temper, then gauss": dict(temper={"sigma_trans": -1.0}, noise={"gauss": torch.zeros(1)}),
    "gauss, then steer": dict(guide={}, temper={"sigma_trans": 1.0}, noise={"expo": torch.zeros(1)}, steer={"every": 0}),
    "steer, then resample_u": dict(steer={}, noise={"resample_u": torch.zeros(1)}),
}


@pytest.mark.parametrize("name", sorted(TWO_ERRORS))
def test_a_call_with_two_bad_arguments_raises_the_first_error(name):
    batch, kw = SC.e2e_batch(), TWO_ERRORS[name]
    with pytest.raises(ValueError) as want:
        _six(batch, CC.NS_E2E, **kw)
    with pytest.raises(ValueError) as got:
        SampleCall.make(batch, CC.NS_E2E, **kw)
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    first = name.split(",")[0]
    assert first in str(want.value), (first, str(want.value))


# ---- fit: B = 4 in two groups of two equal samples, L0 = 20 -------------------------------------------------------------------------
L0, NS = 20, 3


def _twice(v):
    return v.repeat_interleave(2, 0).contiguous()


def _two_group_call():
    g = torch.Generator().manual_seed(20)
    gen = torch.zeros(2, L0, dtype=torch.bool)
    gen[:, 12:18] = True
    resm = torch.ones(2, L0, dtype=torch.bool)
    resm[1, 18:] = False
    batch = {"aa": _twice(torch.randint(0, 20, (2, L0), generator=g)), "generate_mask": _twice(gen), "res_mask": _twice(resm)}
    hot = torch.zeros(2, L0, dtype=torch.bool)
    hot[0, 3], hot[1, 5] = True, True
    start = {"rotmats": _twice(CC._rots(g, 2, L0)), "trans": _twice(torch.randn(2, L0, 3, generator=g)), "seqs": _twice(torch.randint(0, 20, (2, L0), generator=g))}
    noise = {"gauss": torch.randn(NS - 1, 4, L0, 6, generator=g), "resample_u": torch.rand(NS, 2, generator=g, dtype=torch.float64)}
    call = SampleCall.make(batch, NS, True, _twice(torch.rand(2, L0, generator=g) < 0.5), True, t_start=0.4, start=start,
                           aa_allowed=_twice(torch.rand(2, L0, 20, generator=g) < 0.7), noise=noise,
                           guide={"weights": [1.0, 1.0, 0.5, 0.5], "hotspots": _twice(hot), "restraints": [[(12, 3, 4.0, 6.0, 1.0)]] * 2 + [[(13, 2, 3.0, 5.0, 0.5)]] * 2},
                           temper={"seq_temperature": _twice(TC.mixed_tau(2, L0, g)), "sigma_trans": 1.0},
                           steer={"groups": torch.tensor([4, 4, 9, 9]), "lam": 0.3})
    return call, noise


def _fitted_one_by_one(call, Lk, idx):
    return {"grid": call.grid, "flags": call.flags, "cond": sampler.fit_cond(call.cond, L0, Lk, idx), "guide": sampler.fit_guide(call.guide, L0, Lk, idx),
            "temper": sampler.fit_temper(call.temper, L0, Lk, idx), "steer": sampler.fit_steer(call.steer, L0, Lk, idx)}


@pytest.mark.parametrize("Lk,idx", [(32, None), (16, [2, 3]), (32, [2, 3]), (32, [0, 1, 2, 3])])
def test_fit_is_the_four_fit_functions(Lk, idx):
    call, _ = _two_group_call()
    fitted = call.fit(L0, Lk, idx)
    _same(vars(fitted), _fitted_one_by_one(call, Lk, idx), "SampleCall.fit")
    assert fitted is not call and fitted.kinds == call.kinds and all(call.kinds.values())
    B = 4 if idx is None else len(idx)
    assert fitted.cond["res_flags"].shape == (B, Lk) and fitted.guide["hotspots"].shape == (B, Lk) and fitted.temper["tau"].shape == (B, Lk)
    if idx is None:
        assert fitted.steer is call.steer
    elif idx == [2, 3]:
        assert fitted.steer["n_groups"] == 1 and fitted.steer["group_ids"].tolist() == [1]
    assert call.cond["res_flags"].shape == (4, L0), "fit leaves the call it was made from alone"


def test_fit_refuses_a_bucket_that_cuts_a_group():
    call, _ = _two_group_call()
    with pytest.raises(ValueError) as want:
        sampler.fit_steer(call.steer, L0, 32, [1, 2])
    with pytest.raises(ValueError) as got:
        call.fit(L0, 32, [1, 2])
    assert str(got.value) == str(want.value) and "is cut" in str(got.value)


def test_kinds_of_a_plain_call():
    call = SampleCall.make({"aa": torch.zeros(2, 8, dtype=torch.int64)}, 5)
    assert call.kinds == dict.fromkeys(EXTENSIONS, False) and call.flags == (True, True, True) and call.fit(8, 16).kinds == call.kinds
    assert torch.equal(call.grid, sampler.make_grid(5))


# ---- begin: the order of the set-up on a recording stand-in --------------------------------------------------------------------------
class Recorder:
    """stands in for a DeviceSampler: every set-up method appends (its name, its arguments)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not (name.startswith("set_") or name == "init_state"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args))


COMBINATIONS = [c for c in itertools.product((False, True), repeat=4) if c[1] or not c[3]]       # (cond, guide, temper, steer): steer needs guide


def test_there_are_twelve_valid_combinations():
    assert len(COMBINATIONS) == 12


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("on", COMBINATIONS, ids=lambda c: "+".join(k for k, v in zip(EXTENSIONS, c) if v) or "plain")
def test_begin_binds_in_one_order(on, with_ids):
    full, noise = _two_group_call()
    idx = [2, 3]                                                   # a bucket that holds the second group only
    call = SampleCall(full.grid, full.flags, **{k: getattr(full, k) if v else None for k, v in zip(EXTENSIONS, on)}).fit(L0, 32, idx)
    assert call.kinds == dict(zip(EXTENSIONS, on))
    native, gen_mask = ("R1", "x1", "ang1", "seq1"), "gen"
    if not on[3]:
        noise = {k: v for k, v in noise.items() if k != "resample_u"}
    given = dict(noise)
    ids = torch.tensor(idx) + 10 if with_ids else None
    rec = Recorder()
    used = DeviceSampler.begin(rec, call, native, gen_mask, noise, 1234, 10, ids)
    want = [("set_seed", (1234, 10)), ("set_grid", (call.grid,))] + ([("set_sample_ids", (ids,))] if with_ids else []) + \
        [("set_context", native + (gen_mask,))] + ([("set_cond", (call.cond, native))] if on[0] else []) + \
        ([("set_guide", (call.guide,))] if on[1] else []) + ([("set_temper", (call.temper,))] if on[2] else []) + \
        ([("set_steer", (call.steer,))] if on[3] else [])
    assert [n for n, _ in rec.calls] == [n for n, _ in want] + ["init_state"]
    for (name, got), (_, args) in zip(rec.calls, want):
        assert len(got) == len(args) and all(a is b for a, b in zip(got, args)), name
    (state_noise,) = rec.calls[-1][1]
    assert state_noise is used and list(noise) == list(given) and all(noise[k] is given[k] for k in given), "the caller's noise is not touched"
    if on[3]:
        assert call.steer["group_ids"].tolist() == [1]
        assert torch.equal(state_noise["resample_u"], given["resample_u"][:, 1:2]) and state_noise["resample_u"].is_contiguous()
        assert all(state_noise[k] is given[k] for k in given if k != "resample_u")
    else:
        assert state_noise is noise
