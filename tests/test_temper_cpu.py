"""Tempered and stochastic sampling without a GPU: the C ABI, the host-side validation and packing, the helpers that carry a `temper`
through padding / buckets / shards, the Philox and Box-Muller restatement of tests/temper_oracle.py, and the CONDITIONS the GPU tests
(tests/test_gpu_temper.py) rest on -- checked here with the oracle alone, so that those tests cannot pass hollow."""
import ctypes as C
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from pepflowww_amd import _capi, buckets, build, distributed, engine, flow_model, sampler  # noqa: E402
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import temper_cases as TC  # noqa: E402
import temper_oracle as TO  # noqa: E402
from test_lddt_cpu import HEADER  # noqa: E402

CTYPES = {"int": C.c_int, "float": C.c_float, "uint64_t": C.c_uint64, "int64_t": C.c_int64}


def _header_fields(struct):
    """[(name, ctype)] of `typedef struct { ... } struct;` in the header, in order (test_lddt_cpu.header_fields + the 64-bit scalars)"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + struct + ";", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            fields.append((decl.split("*")[-1].strip(), C.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    return fields


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_header_order_and_additive_abi():
    cls = _capi.SamplerTemperArgs
    assert [(n, t) for n, t in cls._fields_] == _header_fields("pf_sampler_temper_args")
    assert [n for n, _ in cls._fields_] == ["pred_logits", "tempered_logits", "tau", "rot_t", "trans_t", "gen_mask", "res_flags", "ts", "step",
                                            "params", "gauss", "seed_dev", "sample_ids", "seed", "first_sample", "B", "L", "num_steps", "sample_bb"]
    assert C.sizeof(cls) == 15 * 8 + 4 * 4 and cls.pred_logits.offset == 0 and cls.seed.offset == 13 * 8 and cls.B.offset == 15 * 8
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65                 # additive: the version stays
    assert f"#define PF_TEMPER_NPARAMS {_capi.TEMPER_NPARAMS}\n" in text and _capi.TEMPER_NPARAMS == 8
    order = [text.index(s) for s in ("int pf_guidance_fwd(", "} pf_sampler_temper_args;", "int pf_sampler_temper(", "int pf_so3_geodesic(")]
    assert order == sorted(order)
    syms = _capi.EXPORTED_SYMBOLS
    assert syms[syms.index("pf_guidance_fwd") + 1] == "pf_sampler_temper"
    src = build.SOURCES
    assert src[src.index("guidance.hip") + 1] == "temper.hip"
    kernel = open(os.path.join(os.path.dirname(HEADER), "..", "pepflowww_amd", "csrc", "temper.hip")).read()
    assert '#include "flow_dev.h"' in kernel and "philox4x32_10(c0" in kernel and "0xD2511F53" not in kernel      # the round function is used, not copied
    assert "asm" not in kernel and "atomic" not in kernel and "powf" not in kernel


def test_library_exports_the_entry_and_refuses_bad_arguments():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_sampler_temper(None, None) == -1
    assert lib.pf_sampler_temper(C.byref(_capi.SamplerTemperArgs()), None) == -1
    buf = (C.c_char * 64)()                              # host memory: a call that got as far as a launch would not return -1

    def args(**kw):
        a = _capi.SamplerTemperArgs()
        for name, typ in _capi.SamplerTemperArgs._fields_:
            setattr(a, name, C.addressof(buf) if typ is C.c_void_p else 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for bad in (dict(step=None), dict(ts=None), dict(num_steps=0), dict(B=0), dict(L=0),
                dict(tau=None, params=None, gauss=None),                                   # nothing to do
                dict(tempered_logits=None), dict(pred_logits=None),                        # tau without its buffers
                dict(rot_t=None), dict(trans_t=None), dict(gen_mask=None),                 # noise with no state
                dict(params=None)):                                                        # gauss without params
        assert lib.pf_sampler_temper(C.byref(args(**bad)), None) == -1, bad


def test_signatures_have_the_new_keyword():
    p = inspect.signature(flow_model.FlowModel._sample_impl).parameters
    assert p["temper"].kind is inspect.Parameter.KEYWORD_ONLY and p["temper"].default is None
    assert inspect.signature(sampler.DeviceSampler.__init__).parameters["temper"].default is False
    assert inspect.signature(engine.DenoiseEngine.sampler).parameters["temper"].default is False
    assert inspect.signature(buckets.BucketedSampler.bind).parameters["temper"].default is None
    assert sampler.TEMPER_DEFAULTS == TO.DEFAULTS


# ---- make_temper ---------------------------------------------------------------------------------------------------------------------
def test_make_temper_packs_and_refuses():
    B, L = 3, 8
    assert sampler.make_temper(None, B, L) is None
    t = sampler.make_temper({}, B, L)
    assert t["tau"] is None and t["params"].dtype == torch.float32 and t["params"].tolist() == [0, 0, 1, 1, 0, 0, 0, 0]
    assert not sampler.temper_has_noise(t) and not sampler.temper_has_noise(None)
    assert sampler.make_temper({"seq_temperature": 1.0}, B, L)["tau"] is None and sampler.make_temper({"seq_temperature": 1}, B, L)["tau"] is None
    t = sampler.make_temper({"seq_temperature": 0.5, "sigma_trans": 1.5, "sigma_rot": 0.25, "power": 2, "t_off": 0.75}, B, L)
    assert t["params"].tolist() == [1.5, 0.25, 2, 0.75, 0, 0, 0, 0] and sampler.temper_has_noise(t)
    assert t["tau"].dtype == torch.float32 and t["tau"].shape == (B, L) and (t["tau"] == 0.5).all()
    row = torch.linspace(0.3, 3.0, L)
    assert torch.equal(sampler.make_temper({"seq_temperature": row}, B, L)["tau"], row.expand(B, L))
    plane = torch.rand(B, L) + 0.1
    assert torch.equal(sampler.make_temper({"seq_temperature": plane.double()}, B, L)["tau"], plane.double().float())
    ones = sampler.make_temper({"seq_temperature": torch.ones(L)}, B, L)["tau"]           # a TENSOR of ones is a plane (only the scalar 1.0 is none)
    assert ones is not None and (ones == 1).all()
    assert sampler.temper_has_noise(sampler.make_temper({"sigma_rot": 0.1}, B, L))
    nan = float("nan")
    bad_plane = plane.clone()
    bad_plane[2, 5] = 0.0
    nan_plane = plane.clone()
    nan_plane[1, 3] = nan
    for bad, match in (({"seq_temperature": 0.0}, "seq_temperature'] = 0.0"),
                       ({"seq_temperature": -1.0}, "-1.0"),
                       ({"seq_temperature": nan}, "nan"),
                       ({"seq_temperature": float("inf")}, "inf"),
                       ({"seq_temperature": "cold"}, "cold"),
                       ({"seq_temperature": True}, "True"),
                       ({"seq_temperature": bad_plane}, "sample 2, residue 5"),
                       ({"seq_temperature": nan_plane}, "sample 1, residue 3"),
                       ({"seq_temperature": torch.ones(L + 1)}, f"[{L}]"),
                       ({"seq_temperature": torch.ones(B, L, 1)}, f"[{B}, {L}]"),
                       ({"seq_temperature": torch.ones(L, dtype=torch.int64)}, "int64"),
                       ({"sigma_trans": -0.1}, "sigma_trans'] = -0.1"),
                       ({"sigma_rot": -1}, "sigma_rot'] = -1"),
                       ({"sigma_trans": nan}, "sigma_trans"),
                       ({"sigma_rot": float("inf")}, "sigma_rot"),
                       ({"sigma_rot": "big"}, "big"),
                       ({"power": 3}, "power'] = 3"),
                       ({"power": 1.5}, "1.5"),
                       ({"power": True}, "True"),
                       ({"t_off": 0.0}, "t_off'] = 0.0"),
                       ({"t_off": 1.5}, "t_off'] = 1.5"),
                       ({"t_off": nan}, "t_off"),
                       ({"temperature": 0.5}, "temperature")):
        with pytest.raises(ValueError, match=re.escape(match)):
            sampler.make_temper(bad, B, L)
    with pytest.raises(ValueError):
        sampler.make_temper([0.5], B, L)


def test_supplied_draws_need_supplied_normals():
    B, L, NS = 2, 8, 4
    noisy, calm = sampler.make_temper({"sigma_trans": 1.0}, B, L), sampler.make_temper({"seq_temperature": 0.5}, B, L)
    expo, gauss = torch.ones(2 * NS, B, L, 20), torch.zeros(NS - 1, B, L, 6)
    with pytest.raises(ValueError, match="gauss"):
        sampler.check_gauss({"expo": expo}, noisy, NS, B, L)
    with pytest.raises(ValueError, match="gauss"):
        sampler.check_gauss({"expo": expo, "gauss": gauss[1:]}, noisy, NS, B, L)          # a wrong shape
    for noise, temper in (({"expo": expo, "gauss": gauss}, noisy), ({"expo": expo}, calm), ({"expo": expo}, None), (None, noisy),
                          ({"trans0": gauss}, noisy)):                                     # without expo the kernel draws
        sampler.check_gauss(noise, temper, NS, B, L)


# ---- padding, buckets, shards --------------------------------------------------------------------------------------------------------
def test_padding_bucket_and_shard_helpers_keep_each_samples_own_entries():
    B, L0, NS = 4, 21, 3
    g = torch.Generator().manual_seed(1)
    plane = TC.mixed_tau(B, L0, g)
    temper = {"seq_temperature": plane, "sigma_trans": 0.5}
    packed = sampler.make_temper(temper, B, L0)
    gauss = torch.randn(NS - 1, B, L0, 6, generator=g)
    noise = {"trans0": torch.randn(B, L0, 3, generator=g), "gauss": gauss, "expo": torch.rand(2 * NS, B, L0, 20, generator=g) + 0.1}
    for Lk in (16, 32):
        n = min(L0, Lk)
        # the reference, stated here: the plane's first n columns, temperature 1 beyond the caller's length
        want = torch.ones(B, Lk)
        want[:, :n] = plane[:, :n]
        fit = sampler.fit_temper(packed, L0, Lk)
        assert torch.equal(fit["tau"], want) and torch.equal(fit["params"], packed["params"])
        sub = buckets.sub_temper(packed, [2, 0], L0, Lk)
        assert torch.equal(sub["tau"], want[[2, 0]]) and torch.equal(sub["params"], packed["params"])
        nz = buckets.sub_noise(noise, [2, 0], L0, Lk)
        wg = torch.zeros(NS - 1, 2, Lk, 6)
        wg[:, :, :n] = gauss[:, [2, 0], :n]
        assert torch.equal(nz["gauss"], wg) and nz["expo"].shape == (2 * NS, 2, Lk, 20) and nz["trans0"].shape == (2, Lk, 3)
    _, padded = flow_model._pad_residues({}, noise, L0, 32)
    wg = torch.zeros(NS - 1, B, 32, 6)
    wg[:, :, :L0] = gauss
    assert torch.equal(padded["gauss"], wg) and torch.equal(padded["expo"][:, :, :L0], noise["expo"]) and (padded["expo"][:, :, L0:] == 1).all()
    assert sampler.fit_temper(None, L0, 32) is None and buckets.sub_temper(None, [0], L0, 16) is None
    no_plane = sampler.make_temper({"sigma_rot": 0.2}, B, L0)
    assert sampler.fit_temper(no_plane, L0, 32)["tau"] is None and buckets.sub_temper(no_plane, [1], L0, 16)["tau"] is None
    # shards: what make_temper packs from the shard's dict is the slice of what it packs from the whole batch's
    for lo, hi in ((0, 2), (1, 4), (3, 4)):
        sh = sampler.shard_temper(temper, lo, hi, B)
        want = TC.shard_temper_ref(temper, lo, hi, B)
        assert torch.equal(sh["seq_temperature"], want["seq_temperature"]) and sh["sigma_trans"] == 0.5
        assert torch.equal(sampler.make_temper(sh, hi - lo, L0)["tau"], packed["tau"][lo:hi])
        sn = distributed.shard_noise(noise, lo, hi)
        assert torch.equal(sn["gauss"], gauss[:, lo:hi]) and torch.equal(sn["expo"], noise["expo"][:, lo:hi]) and torch.equal(sn["trans0"], noise["trans0"][lo:hi])
    shared = {"seq_temperature": plane[0], "sigma_rot": 0.1}
    assert sampler.shard_temper(shared, 1, 3, B)["seq_temperature"] is shared["seq_temperature"]
    assert sampler.shard_temper({"seq_temperature": 0.5}, 1, 3, B) == {"seq_temperature": 0.5}
    assert sampler.shard_temper(None, 0, 1, B) is None


# ---- Philox and Box-Muller -----------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """the Random123 known answers of Philox4x32-10 (the round function of csrc/flow_dev.h)"""
    pi = [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]
    for ctr, key, want in (([0, 0, 0, 0], (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([0xffffffff] * 4, (0xffffffff, 0xffffffff), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           (pi, (0xa4093822, 0x299f31d0), [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        got = TO.philox4x32_10(np.array(ctr, dtype=np.uint32), *key)
        assert got.dtype == np.uint32 and got.tolist() == want, [hex(v) for v in got.tolist()]


def test_counter_layout():
    c = TO.counters(5, 2, [3, (7 << 32) + 9])
    assert c.shape == (2, 5, 2, 4) and c.dtype == np.uint32
    assert c[1, 4, 1].tolist() == [4 * 2 + 1, 0x80000002, 9, 7] and c[0, 0, 0].tolist() == [0, 0x80000002, 3, 0]
    # the categorical draws' counter word 1 is the draw index < 2 * num_steps + 1: the high bit keeps the two streams apart
    assert (c[..., 1] >= 0x80000000).all()


def test_moments_of_the_oracles_normals():
    B, L = TC.abi_case("2x272")["B"], 272
    assert B == 4
    z32 = TO.all_normals(11, [3, 4, 5, 6], L, TC.NS, np.float32)
    z64 = TO.all_normals(11, [3, 4, 5, 6], L, TC.NS, np.float64)
    assert z32.shape == (TC.NS - 1, B, L, 6) and z32.dtype == torch.float32 and z64.dtype == torch.float64
    assert float((z32.double() - z64).abs().max()) < 1e-5 and torch.isfinite(z64).all()
    n = z64.numel()
    for z in (z32.double(), z64):
        assert abs(float(z.mean())) < 5 / math.sqrt(n), float(z.mean())
        # Var(z^2) = E z^4 - 1 = 3 - 1 = 2 for a standard normal: the standard error of the sample variance is sqrt(2 / n)
        assert abs(float((z * z).mean() - z.mean() ** 2) - 1) < 5 * math.sqrt(2 / n), float(z.var())
        rows = z.reshape(-1, 6)
        for i in range(6):
            for j in range(i + 1, 6):
                assert not (rows[:, i] == rows[:, j]).any(), (i, j)
    # another seed, step or sample: other draws; the same sample at another place in the batch: the same draws
    a = TO.normals(11, [3, 4], L, 0)
    assert not np.array_equal(a, TO.normals(12, [3, 4], L, 0)) and not np.array_equal(a, TO.normals(11, [3, 4], L, 1))
    assert np.array_equal(a[::-1], TO.normals(11, [4, 3], L, 0)) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a[:, :100], TO.normals(11, [3, 4], 100, 0))              # the residue index keys the stream, not the length


# ---- the oracle and the conditions of the GPU tests ----------------------------------------------------------------------------------
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_oracle_without_tempering_is_cond_oracle(shape):
    case = TC.abi_case(shape)
    noise = {**case["noise"], "gauss": TC.gauss_of(case["B"], case["L"], TC.NS, 1)}
    kw = dict(encoded=case["encoded"], preds=case["preds"])
    for extra in ({}, {"t_start": 0.5, "start": {"trans": case["gt"][1] + 1.0}, "aa_allowed": CC._allowed("no_cys", case["B"], case["L"], None)}):
        ref = CO.sample(None, case["batch"], noise, TC.NS, case["flags"], **kw, **extra)
        _same(ref, TO.sample(None, case["batch"], noise, TC.NS, case["flags"], temper=None, **kw, **extra))
        # the additions switched off go through the restated loop: the same trajectory, states and draws
        s_a, s_b, r_a, r_b = [], [], [], []
        CO.sample(None, case["batch"], noise, TC.NS, case["flags"], states=s_a, rec=r_a, **kw, **extra)
        _same(ref, TO.sample(None, case["batch"], noise, TC.NS, case["flags"], temper={}, states=s_b, rec=r_b, **kw, **extra))
        _same(ref, TO.sample(None, case["batch"], noise, TC.NS, case["flags"], temper={"seq_temperature": torch.ones(case["L"])}, **kw, **extra))
        assert len(r_a) == len(r_b) == 2 * TC.NS and all(torch.equal(x, y) for x, y in zip(r_a, r_b))
        assert len(s_a) == len(s_b) == TC.NS - 1 and all(torch.equal(x, y) for a, b in zip(s_a, s_b) for x, y in zip(a, b))


def test_free_running_oracle_without_tempering_is_cond_oracle(seeded_sd):
    c = CC.e2e_config(seeded_sd, "L24", "native_t06")
    with torch.no_grad():
        _same(c["ref"], TO.sample(seeded_sd, c["batch"], c["noise"], CC.NS_E2E, encoded=c["encoded"], temper={}, **c["kw"]))


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_cases_cannot_pass_hollow(shape):
    case = TC.abi_case(shape)
    B, L, B0 = case["B"], case["L"], case["B0"]
    gen, resm = case["batch"]["generate_mask"], case["batch"]["res_mask"]
    mov = TC.movable(case)
    # the degenerate samples of the extended shapes
    assert B == CC.ABI_SHAPES[shape][0] + 2 and (gen[B0] == resm[B0]).all(), "a sample with no context row"
    assert gen[B0 + 1].any() and not mov[B0 + 1].any(), "a sample whose backbone switch is off on every row"
    if shape == "3x16":
        assert not gen[1].any(), "a sample without any generated residue"
    assert mov.sum() >= 8 and (gen & ~mov).any() and (~gen).any()
    o = dict(encoded=case["encoded"], preds=case["preds"])
    for name in TC.ALL_CONFIGS:
        c = TC.abi_config(shape, name)
        temper, kw, noise = c["temper"], c["kw"], c["noise"]
        rec, s_t, pre = [], [], []
        ref = TO.sample(None, case["batch"], noise, TC.NS, temper=temper, rec=rec, states=s_t, pre=pre, **o, **kw)
        _same(ref, c["ref"])
        assert CO.min_gap(rec, gen) >= CO.DRAW_GAP, "zero flipped draws is a condition the oracle meets by itself"
        s_p = []
        plain = CO.sample(None, case["batch"], noise, TC.NS, states=s_p, **o, **kw)
        p = TO.params(temper)
        if TO.tau_plane(temper, B, L) is not None:            # the temperature changes some recorded residue type of a generated row
            assert any(not torch.equal(a["seqs"][gen], b["seqs"][gen]) for a, b in zip(ref, plain)), name
            assert all(torch.equal(a["seqs"][~gen], b["seqs"][~gen]) for a, b in zip(ref, plain))
        else:
            assert all(torch.equal(a["seqs"], b["seqs"]) for a, b in zip(ref, plain))
        grid = CO.make_grid(TC.NS, kw.get("t_start"), kw.get("ts"))
        scales = [float(TO.noise_scale(grid, i, temper, torch.float64)) for i in range(TC.NS - 1)]
        if p["sigma_trans"] or p["sigma_rot"]:
            # the state after step 0 differs on some movable row, and on no other row
            for k in (0, 1):
                d = (s_t[0][k] - s_p[0][k]).abs().reshape(B, L, -1).amax(-1)
                assert float(d[mov].max()) > 0.05 and float(d[~mov].max()) == 0, (name, k)
            for k in (2, 3, 4):
                assert torch.equal(s_t[0][k][~gen], s_p[0][k][~gen])
            assert scales[0] > 0
            # the rotation-angle band of cond_oracle still holds on some movable row of every step
            assert all(int((s[5] & mov).sum()) >= 4 for s in s_t), [int((s[5] & mov).sum()) for s in s_t]
        else:
            assert all(torch.equal(x, y) for a, b in zip(s_t, s_p) for x, y in zip(a[:2], b[:2])), "no sigma: the backbone state is the plain run's"
        if name == "null_plane":                              # t_off makes some step noiseless and some step noisy
            assert scales[0] > 0 and scales[1] == 0, scales
            R_in, x_in = pre[1]
            assert torch.equal(R_in, s_t[0][0]) and torch.equal(x_in, s_t[0][1]), "the noiseless step starts from the state as it is"
            assert not torch.equal(pre[0][1][mov], plain[0]["trans"][mov])
    assert TC.abi_config(shape, "null_plane")["temper"].get("seq_temperature") is None
    t = TC.abi_config(shape, "full")["temper"]["seq_temperature"]
    assert t.shape == (B, L) and 0.3 <= float(t.min()) < 0.5 and 2.0 < float(t.max()) <= 3.0


def test_e2e_parameter_sets_have_a_noisy_and_a_noiseless_step():
    grid = CO.make_grid(CC.NS_E2E)
    b = TC.e2e_temper("L24", "b")
    scales = [float(TO.noise_scale(grid, i, b, torch.float64)) for i in range(CC.NS_E2E - 1)]
    assert scales[0] > 0 and scales[1] > 0 and scales[2] == 0, scales
    a = TC.e2e_temper("L64", "a")
    assert all(float(TO.noise_scale(grid, i, a, torch.float64)) > 0 for i in range(CC.NS_E2E - 1))
