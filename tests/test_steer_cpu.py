"""Steered sampling without a GPU: the C ABI, the host-side validation and packing, the helpers that carry a `steer` through buckets and
shards, the properties of the oracle's systematic resampling (tests/steer_oracle.py), and the CONDITIONS the GPU tests
(tests/test_gpu_steer.py) rest on -- margins, non-identity ancestors -- checked here with the oracle alone, so that those tests cannot
pass hollow."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from pepflowww_amd import _capi, buckets, build, distributed, engine, flow_model, geometry, sampler  # noqa: E402
import cond_cases as CC  # noqa: E402
import guide_oracle as GO  # noqa: E402
import steer_cases as SC  # noqa: E402
import steer_oracle as SO  # noqa: E402
import temper_cases as TC  # noqa: E402
import temper_oracle as TO  # noqa: E402
from test_lddt_cpu import HEADER  # noqa: E402
from test_temper_cpu import _header_fields  # noqa: E402


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_header_order_and_additive_abi():
    cls = _capi.SamplerSteerArgs
    assert [(n, t) for n, t in cls._fields_] == _header_fields("pf_sampler_steer_args")    # (pointers of any type are c_void_p there)
    assert C.sizeof(cls) == 23 * 8 + 2 * 8 + 4 * 4 and cls.energy.offset == 0 and cls.seed.offset == 23 * 8 and cls.B.offset == 25 * 8
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65                 # additive: the version stays
    assert f"#define PF_STEER_NPARAMS {_capi.STEER_NPARAMS}\n" in text and _capi.STEER_NPARAMS == 8
    assert f"#define PF_STEER_MAX_GROUP {_capi.STEER_MAX_GROUP}\n" in text and _capi.STEER_MAX_GROUP == 1024
    order = [text.index(s) for s in ("int pf_sampler_temper(", "} pf_sampler_steer_args;", "int pf_sampler_steer(", "int pf_so3_geodesic(")]
    assert order == sorted(order)
    syms = _capi.EXPORTED_SYMBOLS
    assert syms[syms.index("pf_sampler_temper") + 1] == "pf_sampler_steer"
    assert build.SOURCES[build.SOURCES.index("temper.hip") + 1] == "steer.hip"
    kernel = open(os.path.join(os.path.dirname(HEADER), "..", "pepflowww_amd", "csrc", "steer.hip")).read()
    assert "atomic" not in kernel.replace("no atomic", "").replace("there is no atomic", "")


def _args(**kw):
    a = _capi.SamplerSteerArgs()
    one = 8                                                    # (any non-NULL value: every refusal below comes before a launch)
    for k in ("energy", "ts", "step", "params", "group_ptr", "members", "n_groups", "logw", "eprev", "ancestors", "logw_rec", "ess", "code"):
        setattr(a, k, one)
    a.B, a.L, a.num_steps, a.max_group = 4, 16, 3, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_library_exports_the_entry_and_refuses_bad_arguments():
    lib = _capi.load()
    assert lib.pf_sampler_steer(None, None) == -1
    assert lib.pf_sampler_steer(C.byref(_capi.SamplerSteerArgs()), None) == -1
    for bad in ({"params": None}, {"group_ptr": None}, {"members": None}, {"n_groups": None}, {"energy": None}, {"B": 0}, {"L": 0},
                {"num_steps": 0}, {"max_group": 0}, {"B": -1}, {"logw": None}, {"ancestors": None}, {"ess": None}, {"code": None},
                {"ts": None}, {"eprev": None}, {"logw_rec": None},                        # records / grid missing in sampler mode
                {"rot_t": 8}, {"rot_t": 8, "trans_t": 8, "ang_t": 8, "seq_t": 8, "simplex_t": 8, "trans0": 8},      # state only partly given
                {"step": None, "simplex0": 8}):
        assert lib.pf_sampler_steer(C.byref(_args(**bad)), None) == -1, bad
    assert lib.pf_sampler_steer(C.byref(_args(max_group=1025)), None) == -2              # PF_E_TOOLARGE, checked on the host
    assert lib.pf_sampler_steer(C.byref(_args(max_group=1025, step=None)), None) == -2


def test_signatures_have_the_new_keyword():
    assert "steer" in inspect.signature(flow_model.FlowModel._sample_impl).parameters
    assert "steer" in inspect.signature(flow_model.FlowModel._sample_bucketed).parameters
    assert "steer" in inspect.signature(engine.DenoiseEngine.sampler).parameters
    assert "steer" in inspect.signature(sampler.DeviceSampler.__init__).parameters
    assert "steer" in inspect.signature(buckets.BucketedSampler.bind).parameters
    assert "shard_steer" in inspect.getsource(distributed.sample_sharded)
    assert list(inspect.signature(geometry.resample_particles).parameters)[:5] == ["logw", "groups", "u", "ess_frac", "seed"]
    assert sampler.STEER_DEFAULTS == SO.DEFAULTS


# ---- make_steer ------------------------------------------------------------------------------------------------------------------------
def _ctx(B=4, L=8):
    batch = {"aa": torch.zeros(B, L, dtype=torch.int64), "pos": torch.zeros(B, L, 3), "generate_mask": torch.ones(B, L, dtype=torch.bool)}
    guide = sampler.make_guide({"weights": [1, 1, 1, 0]}, B, L)
    return batch, guide


def test_make_steer_packs():
    batch, guide = _ctx()
    assert sampler.make_steer(None, 4, 8, batch, None, guide, None) is None
    st = sampler.make_steer({}, 4, 8, batch, None, guide, None)
    assert st["params"].dtype == torch.float64 and st["params"].tolist() == [1.0, 1.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert st["n_groups"] == 1 and st["max_group"] == 4 and st["members"].tolist() == [0, 1, 2, 3] and st["group_ptr"].tolist() == [0, 4, 4, 4, 4]
    st = sampler.make_steer({"groups": torch.tensor([9, -2, 9, -2]), "lam": 0, "every": 3, "ess_frac": 1, "t_on": 0.25, "t_off": 0.5}, 4, 8, batch, None, guide, None)
    assert st["params"].tolist() == [0.0, 3.0, 1.0, 0.25, 0.5, 0.0, 0.0, 0.0]
    assert st["n_groups"] == 2 and st["members"].tolist() == [0, 2, 1, 3] and st["group_ptr"].tolist() == [0, 2, 4, 4, 4] and st["group_of"].tolist() == [0, 1, 0, 1]
    for m in SO.groups_of([9, -2, 9, -2], 4):
        assert (np.diff(m) > 0).all()
    assert [m.tolist() for m in SO.groups_of([9, -2, 9, -2], 4)] == [[0, 2], [1, 3]]


@pytest.mark.parametrize("bad, match", [
    ({"lamda": 1.0}, "unknown entry 'lamda'"), ({"lam": -1.0}, "lam'. = -1.0"), ({"lam": float("nan")}, "lam'. = nan"), ({"lam": True}, "lam'. = True"),
    ({"lam": float("inf")}, "= inf"), ({"every": 0}, "every'. = 0"), ({"every": 1.5}, "every'. = 1.5"), ({"every": True}, "= True"),
    ({"ess_frac": 1.5}, "ess_frac'. = 1.5"), ({"ess_frac": float("nan")}, "= nan"), ({"ess_frac": -0.1}, "= -0.1"),
    ({"t_on": 0.6, "t_off": 0.5}, "t_on'. = 0.6"), ({"t_off": 1.5}, "t_off'. = 1.5"), ({"t_on": float("nan")}, "= nan"), ({"t_on": -0.5}, "= -0.5"),
    ({"groups": [0, 0, 1, 1]}, "groups"), ({"groups": torch.zeros(3, dtype=torch.int64)}, "groups"), ({"groups": torch.zeros(4)}, "groups"),
    ({"groups": torch.zeros(4, dtype=torch.bool)}, "groups"),
])
def test_make_steer_refuses(bad, match):
    batch, guide = _ctx()
    with pytest.raises(ValueError, match=match):
        sampler.make_steer(bad, 4, 8, batch, None, guide, None)


def test_make_steer_refuses_structure():
    batch, guide = _ctx()
    with pytest.raises(ValueError, match="expected None or a dict"):
        sampler.make_steer([1], 4, 8, batch, None, guide, None)
    with pytest.raises(ValueError, match="steer needs guide"):
        sampler.make_steer({}, 4, 8, batch, None, None, None)
    big, gb = _ctx(1025, 2)
    with pytest.raises(ValueError, match="has 1025 members; at most 1024"):
        sampler.make_steer({}, 1025, 2, big, None, gb, None)
    sampler.make_steer({"groups": torch.arange(1025) % 2}, 1025, 2, big, None, gb, None)
    # exchangeability: the first differing key and the sample pair
    b2 = {k: v.clone() for k, v in batch.items()}
    b2["pos"][2, 3, 1] = 1.0
    with pytest.raises(ValueError, match=r"batch\['pos'\] differs between samples 0 and 2 of group 0"):
        sampler.make_steer({}, 4, 8, b2, None, guide, None)
    sampler.make_steer({"groups": torch.tensor([0, 0, 5, 0])}, 4, 8, b2, None, guide, None)            # sample 2 on its own: fine
    with pytest.raises(ValueError, match=r"batch\['pos'\] differs between samples 1 and 2 of group 7"):
        sampler.make_steer({"groups": torch.tensor([0, 7, 7, 0])}, 4, 8, b2, None, guide, None)
    g2 = sampler.make_guide({"weights": [1, 1, 1, 0], "restraints": [[], [], [], [(0, 1, 1.0, 2.0, 1.0)]]}, 4, 8)
    with pytest.raises(ValueError, match=r"guide\['pair_idx'\] differs between samples 0 and 3"):
        sampler.make_steer({}, 4, 8, batch, None, g2, None)
    tau = torch.ones(4, 8)
    tau[1, 0] = 2.0
    with pytest.raises(ValueError, match=r"temper\['tau'\] differs between samples 0 and 1"):
        sampler.make_steer({}, 4, 8, batch, None, guide, sampler.make_temper({"seq_temperature": tau}, 4, 8))
    flags = torch.ones(4, 8, dtype=torch.bool)
    flags[3, 3] = False
    cond = sampler.make_cond(4, 8, 3, sample_bb=flags)[2]
    with pytest.raises(ValueError, match=r"cond\['res_flags'\] differs between samples 0 and 3"):
        sampler.make_steer({}, 4, 8, batch, cond, guide, None)
    nan = {k: v.clone() for k, v in batch.items()}
    nan["pos"][:, 0, 0] = float("nan")                         # equal NaNs are equal inputs
    sampler.make_steer({}, 4, 8, nan, None, guide, None)


def test_supplied_draws_need_supplied_uniforms():
    batch, guide = _ctx()
    st = sampler.make_steer({"groups": torch.tensor([0, 1, 0, 1])}, 4, 8, batch, None, guide, None)
    expo = torch.ones(6, 4, 8, 20)
    sampler.check_resample_u(None, st, 3)
    sampler.check_resample_u({"expo": None}, st, 3)
    with pytest.raises(ValueError, match="resample_u"):
        sampler.check_resample_u({"expo": expo}, st, 3)
    sampler.check_resample_u({"expo": expo, "resample_u": torch.rand(3, 2)}, st, 3)
    with pytest.raises(ValueError, match=r"expected a tensor \(3, 2\)"):
        sampler.check_resample_u({"resample_u": torch.rand(3, 4)}, st, 3)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        sampler.check_resample_u({"resample_u": torch.ones(3, 2)}, st, 3)
    with pytest.raises(ValueError, match="not steered"):
        sampler.check_resample_u({"resample_u": torch.rand(3, 2)}, None, 3)


def test_bucket_and_shard_helpers_keep_whole_groups():
    batch, guide = _ctx(6, 8)
    lab = torch.tensor([4, 2, 4, 2, 8, 8])
    st = sampler.make_steer({"groups": lab}, 6, 8, batch, None, guide, None)
    assert sampler.fit_steer(st, 8, 16) is st and sampler.fit_steer(None, 8, 16, [0]) is None
    sub = buckets.sub_steer(st, [1, 3, 4, 5], 8, 16)
    assert sub["n_groups"] == 2 and sub["members"].tolist() == [0, 1, 2, 3] and sub["group_ptr"].tolist() == [0, 2, 4, 4, 4]
    assert sub["group_ids"].tolist() == [1, 2] and sub["max_group"] == 2 and torch.equal(sub["params"], st["params"])
    with pytest.raises(ValueError, match="group 0 is cut"):
        buckets.sub_steer(st, [0, 1, 3], 8, 16)
    # shards: a boundary that cuts a group raises and names it
    whole = {"groups": lab, "lam": 2.0}
    assert sampler.shard_steer(None, 0, 3, 6) is None
    out = sampler.shard_steer(whole, 0, 4, 6)
    assert out["groups"].tolist() == [4, 2, 4, 2] and out["lam"] == 2.0 and sampler.steer_groups_of_shard(whole, 0, 4, 6) == [0, 1]
    assert sampler.shard_steer(whole, 4, 6, 6)["groups"].tolist() == [8, 8] and sampler.steer_groups_of_shard(whole, 4, 6, 6) == [2]
    with pytest.raises(ValueError, match=r"shard \[0, 3\) cuts group 2"):
        sampler.shard_steer(whole, 0, 3, 6)
    with pytest.raises(ValueError, match="cuts group 0"):
        sampler.shard_steer({"lam": 1.0}, 0, 3, 6)             # groups = None: the whole batch is one group
    assert sampler.shard_steer({"lam": 1.0}, 0, 6, 6) == {"lam": 1.0}
    noise = {"rot0": torch.zeros(6, 8, 3, 3), "expo": torch.zeros(4, 6, 8, 20), "resample_u": torch.rand(2, 3)}
    nz = distributed.shard_noise(noise, 4, 6)
    assert nz["rot0"].shape[0] == 2 and nz["expo"].shape[1] == 2 and torch.equal(nz["resample_u"], noise["resample_u"])
    assert torch.equal(buckets.sub_noise(noise, [4, 5], 8, 16)["resample_u"], noise["resample_u"])
    assert torch.equal(flow_model._pad_residues({}, noise, 8, 16)[1]["resample_u"], noise["resample_u"])


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def test_philox_uniform_is_its_own_stream():
    u = SO.philox_u((5 << 32) | 17, 3, (1 << 32) + 7)
    out = TO.philox4x32_10(np.array([0, 0xC0000003, 7, 1], dtype=np.uint32), 17, 5)
    assert u == ((int(out[0]) >> 8) + 0.5) * 2.0 ** -24 and 0 < u < 1
    assert SO.philox_u(1, 0, 0) != SO.philox_u(1, 1, 0) != SO.philox_u(1, 1, 1) and SO.philox_u(1, 0, 0) != SO.philox_u(2, 0, 0)
    # the three streams differ in the two high bits of counter word 1
    assert (0xC0000000 | 5) != (0x80000000 | 5) and int(TO.counters(4, 5, [0])[0, 0, 0, 1]) == 0x80000005
    assert SC.U_LO == ((0 >> 8) + 0.5) * 2.0 ** -24 and SC.U_HI == ((0xFFFFFFFF >> 8) + 0.5) * 2.0 ** -24


def test_systematic_counts_and_stable_assignment():
    g = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 64, 257):
        logw = g.normal(size=n) * 1.5
        w = np.exp(logw - logw.max())
        wt = w / w.sum()
        grid = (np.arange(400) + 0.5) / 400
        total = np.zeros(n)
        for u in grid:
            d = SO.decide(np.zeros((n, 5), np.float32), logw, np.zeros(n), 1.0, 1.0, True, True, u)
            c = d["counts"]
            assert d["code"] == 2 and c.sum() == n
            assert ((c == np.floor(n * wt)) | (c == np.ceil(n * wt))).all(), (n, u)
            total += c
            anc, alive = d["anc"], c >= 1
            assert (anc[alive] == np.nonzero(alive)[0]).all(), "a surviving slot keeps its own particle"
            assert alive[anc].all() and not alive[anc != np.arange(n)].any(), "sources survive, destinations are dead"
            assert (np.bincount(anc, minlength=n) == c).all()
            dead = np.nonzero(~alive)[0]
            assert (np.diff(anc[dead]) >= 0).all(), "dead slots in ascending order take the list in ascending order"
            assert (d["logw"] == 0).all() and np.isfinite(d["margin_c"])
        assert np.abs(total / len(grid) - n * wt).max() < 2.0 / len(grid) * n, n      # unbiased: the mean count is n w~ (Riemann sum over u)


def test_decide_update_codes_and_degenerate_cases():
    e = np.array([[1, 2, 3, 4, 5], [0.5, 0, 0, 0, 0], [np.nan, 0, 0, 0, 0]], np.float32)
    d = SO.decide(e, np.zeros(3), np.array([1.0, 0.0, 0.0]), 0.5, 0.0, True, True, 0.5)
    assert d["logw_rec"].tolist() == [-7.0, -0.25, -np.inf] and d["eprev"].tolist() == [15.0, 0.5, 0.0] and d["code"] == 1
    assert (d["anc"] == np.arange(3)).all() and d["logw"].tolist() == d["logw_rec"].tolist()
    off = SO.decide(e, np.array([0.1, 0.2, 0.3]), np.zeros(3), 0.5, 1.0, False, False, 0.5)
    assert off["logw"].tolist() == [0.1, 0.2, 0.3] and off["code"] == 0 and off["eprev"].tolist() == [0, 0, 0]
    dead = SO.decide(e, np.full(3, -np.inf), np.zeros(3), 0.5, 1.0, True, True, 0.5)
    assert dead["code"] == -1 and dead["ess"] == 0 and (dead["anc"] == np.arange(3)).all()
    two = SO.decide(e, np.zeros(3), np.zeros(3), 0.5, 1.0, True, True, 0.5)
    assert two["code"] == 2 and two["anc"][2] != 2 and two["eprev"][2] == two["eprev"][two["anc"][2]]
    # telescoping: after two active steps logw = -lam * E of the second
    lw, pv = np.zeros(2), np.zeros(2)
    for E in ([1.0, 2.0], [0.25, 4.0]):
        d = SO.decide(np.array([[E[0], 0, 0, 0, 0], [E[1], 0, 0, 0, 0]], np.float32), lw, pv, 2.0, 0.0, True, False, 0.5)
        lw, pv = d["logw"], d["eprev"]
    assert lw.tolist() == [-0.5, -8.0]


def test_lineage_against_a_brute_force_walk():
    g = torch.Generator().manual_seed(5)
    for N, B in ((1, 3), (4, 6), (7, 33)):
        anc = torch.randint(0, B, (N, B), generator=g)
        anc[-1] = torch.arange(B)
        lin = sampler.steer_lineage(anc)
        assert lin.dtype == torch.int64 and np.array_equal(lin.numpy(), SO.lineage_brute(anc.numpy()))
        assert torch.equal(lin[-1], torch.arange(B))
    ident = torch.arange(5).expand(3, 5)
    assert torch.equal(sampler.steer_lineage(ident), ident)


def test_oracle_without_steering_is_the_existing_oracles():
    c = TC.abi_config("3x16", "full")
    case = c["case"]
    o = dict(encoded=case["encoded"], preds=case["preds"], **c["kw"])
    a = SO.sample(None, case["batch"], c["noise"], case["NS"], temper=c["temper"], **o)
    b = TO.sample(None, case["batch"], c["noise"], case["NS"], temper=c["temper"], **o)
    import guide_cases as GC
    guide = GC.abi_guide("3x16", "full")
    ga = SO.sample(None, case["batch"], c["noise"], case["NS"], guide=guide, **o)
    gb = GO.sample(None, case["batch"], c["noise"], case["NS"], guide=guide, **o)
    # the combined loop itself: guide + temper with a guide that shifts nothing is the tempered loop
    zero = {**guide, "scale": 0.0}
    za = SO.sample(None, case["batch"], c["noise"], case["NS"], guide=zero, temper=c["temper"], **o)
    # ... and steering that never resamples (ess_frac = 0) changes nothing either
    sa = SO.sample(None, case["batch"], c["noise"], case["NS"], guide=zero, temper=c["temper"],
                   steer={"ess_frac": 0.0, "groups": torch.arange(case["B"]) % 2}, **o)
    for x, y in ((a, b), (ga, gb), (za, b), (sa, b)):
        for i in range(case["NS"]):
            for k in x[i]:
                assert torch.equal(x[i][k], y[i][k]), (i, k)


# ---- the conditions the GPU tests rest on --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, ukind, ess_frac", SC.STANDALONE)
def test_standalone_cases_meet_their_margins(kind, ukind, ess_frac):
    case = SC.standalone_case(kind, ukind, ess_frac)
    ref = SC.standalone_ref(case)
    assert sorted(len(m) for m in case["groups"]) == list(SC.SIZES)
    firsts = [int(m[0]) for m in case["groups"]]
    assert firsts == sorted(firsts) and any((np.diff(m) > 1).any() for m in case["groups"]), "interleaved groups, numbered by first member"
    assert min(ref["margin_c"]) >= SC.MARGIN and min(ref["margin_ess"]) >= SC.MARGIN, (min(ref["margin_c"]), min(ref["margin_ess"]))
    codes = ref["code"]
    if kind == "all_neginf":
        assert set(codes) == {-1} and (ref["ancestors"] == np.arange(case["B"])).all()
    elif ess_frac == 1.0:
        assert set(codes) == {2}
        if kind != "uniform":
            assert (ref["ancestors"] != np.arange(case["B"])).any(), "a case that never moves a particle shows nothing"
        else:
            assert (ref["ancestors"] == np.arange(case["B"])).all()
    else:
        assert {1, 2} <= set(codes) or kind == "uniform", codes
    if ukind in ("lo", "hi"):
        assert {SC.U_LO if ukind == "lo" else SC.U_HI} == set(case["u"][[i for i, m in enumerate(case["groups"]) if len(m) <= 3]].tolist())


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_chain_cases_resample(shape):
    """the chain test feeds the oracle the device's own energies; here the same decisions on the oracle's energies: every group with two
    members moves a particle at some step, and every decision keeps its margin"""
    case = SC.chain_case(shape)
    B, NS = case["B"], case["NS"]
    srec = {}
    noise = {**case["noise"], "gauss": case["gauss"], "resample_u": case["u"]}
    SO.sample(None, case["batch"], noise, NS, case["flags"], guide=SC.CHAIN_GUIDE, temper=SC.CHAIN_TEMPER,
              steer={**SC.CHAIN_STEER, "groups": case["labels"]}, encoded=case["encoded"], preds=case["preds"], srec=srec)
    assert srec["ancestors"].shape == (NS, B) and (srec["ancestors"][:-1] != np.arange(B)).any()
    assert (srec["ancestors"][-1] == np.arange(B)).all() and set(srec["code"][-1].tolist()) == {0}
    assert srec["margin_c"].min() >= SC.MARGIN


def test_e2e_case_meets_the_margin_its_free_decisions_need(seeded_sd):
    """GPU test 5 (d): the oracle's free decisions equal the device's only if no tolerated deviation of the recorded energies can move a
    decision: steer_cases.weight_shift_bound, with the per-term tolerance of tests/test_gpu_guide.py summed over the five terms"""
    from test_gpu_guide import _energy_tolerance
    c = SC.e2e_case(seeded_sd)
    srec = c["srec"]
    tol = _energy_tolerance(c["batch"], c["guide"], c["energy"], c["xs"]).sum(-1).max(1).values.numpy()       # [NS]: the largest of a step
    need = np.array([SC.weight_shift_bound(SC.E2E_LAM, tol[s], tol[s - 1] if s else 0.0) for s in range(len(tol))])
    margin = srec["margin_c"][:, 0]
    print(f"e2e: margins {margin.tolist()}, needed {need.tolist()}, tolerance of E {tol.tolist()}; codes {srec['code'].ravel().tolist()}")
    assert (margin[:-1] > need[:-1]).all()
    assert (srec["ancestors"][0] != np.arange(SC.E2E_B)).any(), "a case that never moves a particle shows nothing"
    assert set(srec["code"][:-1].ravel().tolist()) == {2} and srec["code"][-1].tolist() == [0]
