"""Guided sampling without a GPU: the oracle against cond_oracle, the host-side validation and packing, the helpers that carry a
guide through padding / buckets / shards, the C ABI, and the CONDITIONS the GPU tests (tests/test_gpu_guide.py) rest on -- checked
here with the oracle alone, so that those tests cannot pass hollow."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from pepflowww_amd import _capi, buckets, build, flow_model, sampler  # noqa: E402
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import guide_cases as GC  # noqa: E402
import guide_oracle as GO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_oracle_without_guide_and_with_zero_weights_is_cond_oracle(shape):
    case = GC.abi_case(shape)
    kw = dict(encoded=case["encoded"], preds=case["preds"])
    for extra in ({}, {"t_start": 0.5, "start": {"trans": case["gt"][1] + 1.0}, "aa_allowed": CC._allowed("no_cys", case["B"], case["L"], None)}):
        ref = CO.sample(None, case["batch"], case["noise"], case["NS"], case["flags"], **kw, **extra)
        _same(ref, GO.sample(None, case["batch"], case["noise"], case["NS"], case["flags"], guide=None, **kw, **extra))
        full = GC.abi_guide(shape, "full")
        zero = {**full, "weights": [0.0] * 4, "restraints": [[(i, j, lo, hi, 0.0) for (i, j, lo, hi, w) in rs] for rs in full["restraints"]]}
        grec = []
        _same(ref, GO.sample(None, case["batch"], case["noise"], case["NS"], case["flags"], guide=zero, grec=grec, **kw, **extra))
        assert len(grec) == case["NS"] and all(float(e.abs().max()) == 0 and float(n.max()) == 0 for e, n, _ in grec)
    rec_a, rec_b = [], []
    CO.sample(None, case["batch"], case["noise"], case["NS"], case["flags"], rec=rec_a, **kw)
    GO.sample(None, case["batch"], case["noise"], case["NS"], case["flags"], guide=GC.abi_guide(shape, "full"), rec=rec_b, **kw)
    assert len(rec_a) == len(rec_b) == 2 * case["NS"]                     # the same draws, in the same order


def test_free_running_oracle_without_guide_is_cond_oracle(seeded_sd):
    c = CC.e2e_config(seeded_sd, "L24", "native_t06")
    with torch.no_grad():
        got = GO.sample(seeded_sd, c["batch"], c["noise"], CC.NS_E2E, encoded=c["encoded"], guide=None, **c["kw"])
    _same(c["ref"], got)


def test_autograd_gradient_agrees_with_a_central_difference():
    """the oracle's own yardstick: float64 autograd against a finite difference of the float64 energy, on the rows the kernel moves"""
    case = GC.abi_case("3x16")
    guide = GC.abi_guide("3x16", "full")
    x, _ = GC.abi_x(case)
    cls = GO.row_classes(case["batch"]["generate_mask"], case["batch"]["res_mask"], case["flags"][0], guide["hotspots"])
    _, g = GO.potential(x, cls, guide)
    rows = cls["M"].nonzero()[:6].tolist()
    h = 1e-6
    for b, l in rows:
        for k in range(3):
            xp, xm = x.double().clone(), x.double().clone()
            xp[b, l, k] += h
            xm[b, l, k] -= h
            fd = float((GO.energies(xp, cls, guide).sum() - GO.energies(xm, cls, guide).sum()) / (2 * h))
            assert abs(fd - float(g[b, l, k])) <= 1e-5 * max(1.0, abs(fd)), (b, l, k, fd, float(g[b, l, k]))
    assert float(g[~cls["M"]].abs().max()) == 0


# ---- the conditions of the GPU tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_cases_exercise_every_term_the_clip_and_the_degenerate_samples(shape):
    case = GC.abi_case(shape)
    B, L, B0 = case["B"], case["L"], case["B0"]
    gen, resm = case["batch"]["generate_mask"], case["batch"]["res_mask"]
    guide = GC.abi_guide(shape, "full")
    cls = GO.row_classes(gen, resm, case["flags"][0], guide["hotspots"])
    # the degenerate samples
    assert not cls["C"][B0].any() and cls["P"][B0].any(), "a sample with no context row"
    assert cls["P"][B0 + 1].any() and not cls["M"][B0 + 1].any(), "a sample with a peptide and no movable row"
    assert not cls["H"][B0 + 1].any() and cls["H"][0].any(), "a sample with no hot spot beside samples with some"
    assert GC.abi_guide(shape, "null_plane").get("hotspots") is None
    assert len(guide["restraints"][0]) == GO.MAX_PAIRS and guide["restraints"][B0] == []
    if shape == "3x16":
        assert not cls["P"][1].any(), "a sample without any peptide row"
    grid = CO.make_grid(case["NS"])
    p = GO.params(guide)
    positive = torch.zeros(5, dtype=torch.bool)
    clipped = free = 0
    for step in range(case["NS"]):
        x = torch.where(cls["M"][..., None], case["preds"][step][1], case["gt"][1])
        res = cls["P"] | cls["C"]
        d = torch.cdist(x.double(), x.double()) + 10.0 * torch.eye(L)
        assert float(d[res[:, :, None] & res[:, None, :]].min()) > 1e-3, "no pair below 1e-3 Angstrom"
        _, e, g, n = GO.guided(case["preds"][step][1], case["gt"][1], cls, guide, grid[step])
        positive |= (e > 0).any(0)
        raw = float(GO.schedule(grid[step], p)) * g.norm(dim=-1)             # |lambda g| before the clip
        clipped += int(((raw > p["max_shift"] * 1.01) & cls["M"]).sum())
        free += int(((raw < p["max_shift"] * 0.99) & (raw > 0) & cls["M"]).sum())
        assert float(n.max()) <= p["max_shift"] * (1 + 1e-12)
    assert positive.all(), positive
    assert clipped >= 1 and free >= 1, (clipped, free)


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
def test_descent_case_lowers_the_energy(shape):
    case = GC.abi_case(shape)
    guide = GC.descent_guide(shape)
    cls = GO.row_classes(case["batch"]["generate_mask"], case["batch"]["res_mask"], case["flags"][0], guide["hotspots"])
    out, e, _, n = GO.guided(case["preds"][0][1], case["gt"][1], cls, guide, 1.0)
    after = GO.energies(torch.where(cls["M"][..., None], out, case["gt"][1].double()), cls, guide)
    moved = cls["M"].any(1)
    assert moved.sum() >= 2 and float(n.max()) > 0
    assert (after.sum(1)[moved] < e.sum(1)[moved]).all(), (e.sum(1), after.sum(1))
    assert torch.equal(after.sum(1)[~moved], e.sum(1)[~moved])


# ---- make_guide ----------------------------------------------------------------------------------------------------------------------
def test_make_guide_packs_and_refuses():
    B, L = 3, 8
    gen = torch.zeros(B, L, dtype=torch.bool)
    gen[:, 5:] = True
    resm = torch.ones(B, L, dtype=torch.bool)
    resm[:, -1] = False
    hot = torch.zeros(L, dtype=torch.bool)
    hot[1] = True
    assert sampler.make_guide(None, B, L) is None
    g = sampler.make_guide({"weights": {"hotspot": 2.0, "ca_bond": 0.5}, "hotspots": hot, "restraints": [(5, 6, 3.0, 4.0, 1.5)], "power": 2, "t_on": 0.25},
                           B, L, gen, resm)
    assert g["params"].dtype == torch.float32 and g["params"].tolist() == [0, 0, 0.5, 2.0, 4.5, 4.5, 3, torch.tensor(0.1).item(), 8.0, 1.0, 1.0, 0.25, 2, 2.0, 0, 0]
    assert g["hotspots"].dtype == torch.uint8 and g["hotspots"].shape == (B, L) and g["hotspots"].sum() == B
    assert g["pair_idx"].shape == (B, 64, 2) and g["pair_idx"].dtype == torch.int32 and g["pair_par"].shape == (B, 64, 3)
    assert g["pair_idx"][2, 0].tolist() == [5, 6] and g["pair_par"][2, 0].tolist() == [3.0, 4.0, 1.5] and float(g["pair_par"][:, 1:].abs().max()) == 0
    per = sampler.make_guide({"restraints": [[], [(0, 1, 1.0, 2.0, 1.0)], []]}, B, L)
    assert per["hotspots"] is None and per["pair_par"][:, 0, 2].tolist() == [0.0, 1.0, 0.0]
    assert sampler.make_guide({"restraints": [[], [], []]}, B, L)["pair_par"].abs().max() == 0
    assert sampler.make_guide({"restraints": [(0, 1, 1.0, 2.0, 1.0)] * 64}, B, L)["pair_par"][:, :, 2].min() == 1.0
    hot_gen = hot.clone()
    hot_gen[6] = True
    for bad, match in (({"hotspots": hot_gen}, "residue 6 is a generated"),
                       ({"restraints": [(0, L, 1.0, 2.0, 1.0)]}, f"index {L}"),
                       ({"restraints": [(-1, 2, 1.0, 2.0, 1.0)]}, "index -1"),
                       ({"restraints": [(0, L - 1, 1.0, 2.0, 1.0)]}, f"index {L - 1}"),          # a masked residue
                       ({"restraints": [(0, 1, 3.0, 2.0, 1.0)]}, "lo = 3.0 > hi = 2.0"),
                       ({"restraints": [(0, 1, 1.0, 2.0, -0.5)]}, "weight -0.5"),
                       ({"weights": {"self_clash": -1.0}}, "-1.0"),
                       ({"weights": [1.0, 1.0, 1.0]}, "got 3"),
                       ({"weights": {"restraint": 1.0}}, "restraint"),
                       ({"power": 3}, "power'] = 3"),
                       ({"power": 1.5}, "1.5"),
                       ({"t_on": 1.0}, "t_on'] = 1.0"),
                       ({"beta": 0.0}, "beta"),
                       ({"restraints": [(0, 1, 1.0, 2.0, 1.0)] * 65}, "65 restraints"),
                       ({"restraints": [[], []]}, "per sample"),
                       ({"radius": 3.0}, "radius")):
        with pytest.raises(ValueError, match=re.escape(match)):
            sampler.make_guide(bad, B, L, gen, resm)
    with pytest.raises(ValueError):
        sampler.make_guide([1, 2], B, L)


# ---- padding, buckets, shards --------------------------------------------------------------------------------------------------------
def test_padding_bucket_and_shard_helpers_keep_each_samples_own_entries():
    B, L0 = 4, 21
    g = torch.Generator().manual_seed(1)
    hot = torch.rand(B, L0, generator=g) < 0.3
    restraints = [[(b, b + 1, 1.0 + b, 2.0 + b, 0.5 + b)] * (b + 1) for b in range(B)]
    guide = {"weights": [1.0, 0.0, 0.0, 1.0], "hotspots": hot, "restraints": restraints}
    packed = sampler.make_guide(guide, B, L0)
    for Lk in (16, 32):
        n = min(L0, Lk)
        fit = sampler.fit_guide(packed, L0, Lk)
        assert fit["hotspots"].shape == (B, Lk) and torch.equal(fit["hotspots"][:, :n].bool(), hot[:, :n]) and not fit["hotspots"][:, L0:].any()
        assert torch.equal(fit["pair_idx"], packed["pair_idx"]) and torch.equal(fit["params"], packed["params"])
        sub = buckets.sub_guide(packed, [2, 0], L0, Lk)
        assert torch.equal(sub["hotspots"][:, :n].bool(), hot[[2, 0], :n]) and sub["hotspots"].shape == (2, Lk)
        assert torch.equal(sub["pair_idx"], packed["pair_idx"][[2, 0]]) and torch.equal(sub["pair_par"], packed["pair_par"][[2, 0]])
        assert sub["pair_idx"][0, 0].tolist() == [2, 3] and int((sub["pair_par"][0, :, 2] > 0).sum()) == 3       # residue indices unchanged
    assert sampler.fit_guide(None, L0, 32) is None and buckets.sub_guide(None, [0], L0, 16) is None
    no_plane = sampler.make_guide({"restraints": restraints[0]}, B, L0)
    assert sampler.fit_guide(no_plane, L0, 32)["hotspots"] is None
    # shards: what make_guide packs from the shard's dict is the slice of what it packs from the whole batch's
    for lo, hi in ((0, 2), (1, 4), (3, 4)):
        sh = sampler.shard_guide(guide, lo, hi, B)
        want = GC.shard_guide_ref(guide, lo, hi, B)
        assert torch.equal(sh["hotspots"], want["hotspots"]) and sh["restraints"] == want["restraints"] and sh["weights"] == guide["weights"]
        ps = sampler.make_guide(sh, hi - lo, L0)
        for k in ("hotspots", "pair_idx", "pair_par"):
            assert torch.equal(ps[k], packed[k][lo:hi]), (k, lo, hi)
    shared = {"hotspots": hot[0], "restraints": restraints[1]}
    sh = sampler.shard_guide(shared, 1, 3, B)
    assert sh["hotspots"] is shared["hotspots"] and sh["restraints"] is shared["restraints"]
    assert sampler.shard_guide(None, 0, 1, B) is None


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_header_order_and_additive_abi():
    cls = _capi.GuidanceArgs
    assert [(n, t) for n, t in cls._fields_] == header_fields("pf_guidance_args")
    assert C.sizeof(cls) == 17 * 8 + 4 * 4 and cls.pred_trans.offset == 0 and cls.error.offset == 16 * 8 and cls.B.offset == 17 * 8
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65                 # additive: the version stays
    for name, val in (("PF_GUIDE_MAX_PAIRS", _capi.GUIDE_MAX_PAIRS), ("PF_GUIDE_MAX_L", _capi.GUIDE_MAX_L),
                      ("PF_GUIDE_NPARAMS", _capi.GUIDE_NPARAMS), ("PF_GUIDE_NTERMS", _capi.GUIDE_NTERMS)):
        assert f"#define {name} {val}\n" in text, name
    assert _capi.GUIDE_MAX_PAIRS == 64 == GO.MAX_PAIRS and _capi.GUIDE_MAX_L >= 400 and _capi.GUIDE_NTERMS == len(sampler.GUIDE_TERMS) == 5
    assert sampler.GUIDE_TERMS == GO.TERMS and sampler.GUIDE_DEFAULTS == GO.DEFAULTS
    order = [text.index(s) for s in ("int pf_sampler_step_cond(", "} pf_guidance_args;", "int pf_guidance_fwd(", "int pf_so3_geodesic(")]
    assert order == sorted(order)
    syms = _capi.EXPORTED_SYMBOLS
    assert syms[syms.index("pf_sampler_step_cond") + 1] == "pf_guidance_fwd"
    src = build.SOURCES
    assert src[src.index("flow_step.hip") + 1] == "guidance.hip"
    kernel = open(os.path.join(os.path.dirname(HEADER), "..", "pepflowww_amd", "csrc", "guidance.hip")).read()
    assert "asm" not in kernel and "atomic" not in kernel.replace("no atomics", "")


def test_library_exports_the_entry_and_refuses_bad_arguments():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_guidance_fwd(None, None) == -1
    assert lib.pf_guidance_fwd(C.byref(_capi.GuidanceArgs()), None) == -1
    buf = (C.c_char * 64)()                              # host memory: a call that got as far as a launch would not return -1 / -2

    def args(**kw):
        a = _capi.GuidanceArgs()
        for name, typ in _capi.GuidanceArgs._fields_:
            setattr(a, name, C.addressof(buf) if typ is C.c_void_p else 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for bad in (dict(pred_trans=None), dict(trans1=None), dict(gen_mask=None), dict(res_mask=None), dict(params=None), dict(energy=None),
                dict(B=0), dict(L=0), dict(pair_idx=None), dict(pair_par=None), dict(ts=None), dict(num_steps=0), dict(guided_trans=None),
                dict(shift_max=None), dict(step=None, t=None)):
        assert lib.pf_guidance_fwd(C.byref(args(**bad)), None) == -1, bad
    assert lib.pf_guidance_fwd(C.byref(args(L=_capi.GUIDE_MAX_L + 1)), None) == -2
    assert lib.pf_guidance_fwd(C.byref(args(L=_capi.GUIDE_MAX_L + 1, step=None)), None) == -2


def test_sample_and_sampler_signatures_have_the_new_keyword():
    p = inspect.signature(flow_model.FlowModel._sample_impl).parameters
    assert p["guide"].kind is inspect.Parameter.KEYWORD_ONLY and p["guide"].default is None
    assert inspect.signature(sampler.DeviceSampler.__init__).parameters["guide"].default is False
    from pepflowww_amd import geometry
    q = inspect.signature(geometry.ca_potential).parameters
    assert list(q)[:6] == ["x", "peptide", "movable", "context", "hotspots", "restraints"]
