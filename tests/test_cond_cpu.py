"""Conditioned sampling (partial start, per-residue switches, allowed residue types) without a GPU: the oracle against O.sample, the
host helpers' validation and packing, the C ABI (struct layout, exports, argument checks), the index plumbing of padding, buckets and
shards, and the draw-gap condition of every committed case."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from oracle import pepflow_oracle as O  # noqa: E402
from pepflowww_amd import _capi, buckets, flow_model, sampler, synth  # noqa: E402
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pepflow_hip.h")


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_with_defaults_is_the_reference_loop(seeded_sd):
    B, L, NS = 2, 16, 3
    batch = synth.make_pocket_batch(B, L, 5, seed=99)
    noise = synth.make_noise(B, L, NS, seed=2)
    with torch.no_grad():
        ref = O.sample(seeded_sd, batch, noise, NS)
        got = CO.sample(seeded_sd, batch, noise, NS)
        same = CO.sample(seeded_sd, batch, noise, NS, t_start=1e-2, aa_allowed=torch.ones(20, dtype=torch.bool),
                         flags=(torch.ones(B, L, dtype=torch.bool), True, True))
    assert len(ref) == len(got) == NS
    for r, g, s in zip(ref, got, same):
        assert set(r) == set(g)
        for k in r:
            assert torch.equal(r[k], g[k]), k
            assert torch.equal(r[k], s[k]), k       # all classes allowed / constant planes / the default t_start: the same loop


def test_oracle_mask_and_flags():
    """the draws stay inside the allowed set; a switched-off row keeps the context in its channel"""
    c = CC.abi_config("3x16", "mixed_random")
    gen = c["case"]["batch"]["generate_mask"]
    fb, fa, fs = c["kw"]["flags"]
    R1, x1, ang1, seq1 = c["case"]["gt"]
    for t in c["ref"]:
        rows = gen & fs
        assert c["kw"]["aa_allowed"][rows].gather(-1, t["seqs"][rows][:, None]).all()
        assert torch.equal(t["seqs"][~rows], seq1[~rows])
        assert torch.equal(t["trans"][~(gen & fb)], x1[~(gen & fb)]) and torch.equal(t["angles"][~fa], ang1[~fa])
    assert (gen & fs).any() and (gen & ~fs).any() and (gen & ~fb).any() and (gen & ~fa).any()


@pytest.mark.parametrize("shape", list(CC.ABI_SHAPES))
@pytest.mark.parametrize("name", list(CC.ABI_CONFIGS))
def test_abi_cases_keep_every_draw_away_from_its_boundary(shape, name):
    c = CC.abi_config(shape, name)
    rec = []
    CO.sample(None, c["case"]["batch"], c["noise"], c["case"]["NS"], encoded=c["case"]["encoded"], preds=c["case"]["preds"], rec=rec, **c["kw"])
    assert len(rec) == 2 * c["case"]["NS"]
    assert CO.min_gap(rec, c["case"]["batch"]["generate_mask"]) >= CO.DRAW_GAP


def test_abi_cases_cover_what_they_claim():
    for shape, (B, L, empty) in CC.ABI_SHAPES.items():
        case = CC.abi_case(shape)
        gen = case["batch"]["generate_mask"]
        assert gen.shape == (B, L) and (empty is None or not gen[empty].any()) and gen.any(1).sum() == B - (empty is not None)
        raw = torch.stack([p[2] for p in case["preds"]])
        assert (raw < 0).any() and (raw > 2 * torch.pi).any()
        th = torch.linalg.norm(O.so3_calc_vf(case["noise"]["rot0"], case["start"]["rotmats"]), dim=-1)
        assert th.min() > CO.ROT_ANGLE_MIN - 1e-3 and th.max() < CO.ROT_ANGLE_MAX + 1e-3


@pytest.mark.parametrize("shape", list(CC.E2E_SHAPES))
@pytest.mark.parametrize("name", CC.E2E_CONFIGS)
def test_end_to_end_cases_keep_every_draw_away_from_its_boundary(seeded_sd, shape, name):
    """every end-to-end case (the oracle's network on the CPU: a second or two each).  traj_start is built here on the oracle's own first
    run; the GPU test, which starts from the DEVICE's first run, widens and asserts again on that start."""
    c = CC.e2e_config(seeded_sd, shape, name)
    rec = []
    with torch.no_grad():
        CO.sample(seeded_sd, c["batch"], c["noise"], CC.NS_E2E, encoded=c["encoded"], rec=rec, **c["kw"])
    assert CO.min_gap(rec, c["batch"]["generate_mask"]) >= CO.DRAW_GAP


# ---- host helpers ---------------------------------------------------------------------------------------------------------------------
def test_grid():
    assert torch.equal(sampler.make_grid(7), torch.linspace(1e-2, 1.0, 7))
    assert torch.equal(sampler.make_grid(7, t_start=1e-2), torch.linspace(1e-2, 1.0, 7))
    assert torch.equal(sampler.make_grid(5, t_start=0.6), torch.linspace(0.6, 1.0, 5))
    g = sampler.make_grid(3, ts=[0.3, 0.35, 1.0])
    assert g.dtype == torch.float32 and g.tolist() == torch.tensor([0.3, 0.35, 1.0]).tolist()
    for bad in (0.0, -0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            sampler.make_grid(4, t_start=bad)
    for bad in ([0.5, 0.4, 1.0], [0.5, 0.5, 1.0], [0.0, 0.5, 1.0], [0.2, 0.5, 1.1], [0.2, 1.0], [[0.2, 0.5, 1.0]], [0.2, float("nan"), 1.0]):
        with pytest.raises(ValueError):
            sampler.make_grid(3, ts=bad)
    with pytest.raises(ValueError):
        sampler.make_grid(3, t_start=0.5, ts=[0.5, 0.7, 1.0])


def test_flag_bytes():
    B, L = 2, 5
    assert sampler.pack_res_flags(True, False, True, B, L) == ((True, False, True), None)
    bb = torch.zeros(B, L, dtype=torch.bool)
    bb[0, 1] = True
    sq = torch.zeros(B, L, dtype=torch.bool)
    sq[1, 4] = sq[0, 1] = True
    flags, plane = sampler.pack_res_flags(bb, True, sq, B, L)
    assert flags == (True, True, True) and plane.dtype == torch.uint8 and plane.shape == (B, L)
    want = torch.full((B, L), 2, dtype=torch.uint8)
    want[0, 1], want[1, 4] = 7, 6
    assert torch.equal(plane, want)
    assert torch.equal(sampler.pack_res_flags(bb, False, False, B, L)[1], bb.to(torch.uint8))
    for bad in (torch.zeros(B, L + 1, dtype=torch.bool), torch.zeros(L, dtype=torch.bool), torch.zeros(B, L)):
        with pytest.raises(ValueError):
            sampler.pack_res_flags(True, bad, True, B, L)


def test_allowed_bits():
    B, L = 2, 3
    assert sampler.pack_aa_allowed(None, B, L) is None
    m = torch.ones(20, dtype=torch.bool)
    m[CC.CYS] = False
    bits = sampler.pack_aa_allowed(m, B, L)
    assert bits.dtype == torch.int32 and bits.shape == (B, L) and (bits == sampler.ALL_AA - 2).all()
    per = torch.zeros(L, 20, dtype=torch.bool)
    per[0, 0] = per[1, 19] = per[2, 3] = per[2, 4] = True
    assert sampler.pack_aa_allowed(per, B, L).tolist() == [[1, 1 << 19, 24]] * B
    full = torch.rand(B, L, 20, generator=torch.Generator().manual_seed(1)) < 0.5
    full[..., 7] = True
    bits = sampler.pack_aa_allowed(full, B, L)
    assert all(bool(bits[b, l] >> k & 1) == bool(full[b, l, k]) for b in range(B) for l in range(L) for k in range(20))
    full[1, 2] = False
    with pytest.raises(ValueError, match="sample 1, residue 2"):
        sampler.pack_aa_allowed(full, B, L)
    for bad in (torch.ones(19, dtype=torch.bool), torch.ones(B, 20, dtype=torch.bool), torch.ones(B, L, 20), torch.ones(1, B, L, 20, dtype=torch.bool)):
        with pytest.raises(ValueError):
            sampler.pack_aa_allowed(bad, B, L)


def _start(B, L):
    return {"rotmats": torch.eye(3).expand(B, L, 3, 3).clone(), "trans": torch.zeros(B, L, 3), "angles": torch.zeros(B, L, 5),
            "seqs": torch.zeros(B, L, dtype=torch.int64), "seqs_simplex": torch.zeros(B, L, 20), "rotmats_1": torch.zeros(B, L, 3, 3)}


def test_start_dict_and_make_cond():
    B, L, N = 2, 4, 3
    assert sampler.check_start(None, B, L) is None and sampler.check_start("native", B, L) == {}
    st = sampler.check_start(_start(B, L), B, L)
    assert set(st) == {"rotmats", "trans", "angles", "seqs"} and st["seqs"].dtype == torch.int64 and st["trans"].dtype == torch.float32
    assert set(sampler.check_start({"trans": torch.zeros(B, L, 3, dtype=torch.float64)}, B, L)) == {"trans"}
    for key, bad in (("rotmats", torch.zeros(B, L, 9)), ("trans", torch.zeros(B, L + 1, 3)), ("angles", torch.zeros(B, L, 7)),
                     ("seqs", torch.zeros(B, L)), ("seqs", torch.zeros(B, dtype=torch.int64)), ("trans", torch.zeros(B, L, 3, dtype=torch.int64)),
                     ("trans", [[0.0]])):
        with pytest.raises(ValueError):
            sampler.check_start(dict(_start(B, L), **{key: bad}), B, L)
    for bad in (-1, 22):                                                 # 0..19 and UNK / PAD (20, 21) pass, nothing else
        seqs = torch.full((B, L), 21, dtype=torch.int64)
        seqs[1, 2] = bad
        with pytest.raises(ValueError, match="0..21"):
            sampler.check_start({"seqs": seqs}, B, L)
    assert sampler.check_start({"seqs": torch.tensor([[0, 19, 20, 21]] * B)}, B, L)["seqs"].tolist() == [[0, 19, 20, 21]] * B
    for bad in ("noise", 3, [1]):
        with pytest.raises(ValueError):
            sampler.check_start(bad, B, L)
    # make_cond: a call without the new arguments has no conditioning and the reference's grid
    grid, flags, cond = sampler.make_cond(B, L, N, True, False, True)
    assert cond is None and flags == (True, False, True) and torch.equal(grid, torch.linspace(1e-2, 1.0, N))
    grid, flags, cond = sampler.make_cond(B, L, N, t_start=0.25)
    assert cond is None and torch.equal(grid, torch.linspace(0.25, 1.0, N))              # a grid alone: still pure noise
    for st in ("native", _start(B, L)):
        with pytest.raises(ValueError, match="t_start or ts"):
            sampler.make_cond(B, L, N, start=st)
    _, _, cond = sampler.make_cond(B, L, N, start="native", ts=[0.5, 0.7, 1.0])
    assert cond == {"partial": True}
    _, flags, cond = sampler.make_cond(B, L, N, torch.ones(B, L, dtype=torch.bool), aa_allowed=torch.ones(20, dtype=torch.bool))
    assert flags == (True, True, True) and not cond["partial"] and set(cond) == {"partial", "res_flags", "aa_allowed"}


def test_padding_buckets_and_shards_carry_the_conditioning():
    B, L0, N = 3, 20, 2
    g = torch.Generator().manual_seed(0)
    st = _start(B, L0)
    st["trans"] = torch.randn(B, L0, 3, generator=g)
    fl = torch.rand(B, L0, generator=g) < 0.5
    al = torch.rand(B, L0, 20, generator=g) < 0.7
    al[..., 0] = True
    _, _, cond = sampler.make_cond(B, L0, N, fl, True, False, t_start=0.5, start=st, aa_allowed=al)
    batch = synth.make_pocket_batch(B, L0, 4, seed=3)
    noise = synth.make_noise(B, L0, N, seed=1)
    ob, nz = flow_model._pad_residues(batch, noise, L0, 32)             # (its contract is unchanged: the conditioning is padded beside it)
    assert ob["aa"].shape == (B, 32) and nz["rot0"].shape == (B, 32, 3, 3)
    pc = sampler.fit_cond(cond, L0, 32)
    assert pc["partial"] and set(pc) == set(cond)
    for k in sampler.COND_ROW_KEYS:
        assert pc[k].shape[:2] == (B, 32) and pc[k].dtype == cond[k].dtype and torch.equal(pc[k][:, :L0], cond[k]), k
    # inert rows: no flag, every class, identity frame, zeros, residue type 21
    assert (pc["res_flags"][:, L0:] == 0).all() and (pc["aa_allowed"][:, L0:] == sampler.ALL_AA).all() and (pc["seqs"][:, L0:] == 21).all()
    assert torch.equal(pc["rotmats"][:, L0:], torch.eye(3).expand(B, 12, 3, 3)) and (pc["trans"][:, L0:] == 0).all() and (pc["angles"][:, L0:] == 0).all()
    # buckets: samples [2, 0] cut to 16 / padded to 48
    for Lk in (16, 48):
        sc = buckets.sub_cond(cond, [2, 0], L0, Lk)
        n = min(L0, Lk)
        for k in sampler.COND_ROW_KEYS:
            assert sc[k].shape[:2] == (2, Lk) and torch.equal(sc[k][:, :n], cond[k][[2, 0], :n]), (k, Lk)
        assert (sc["res_flags"][:, L0:] == 0).all() and (sc["aa_allowed"][:, L0:] == sampler.ALL_AA).all()
    assert buckets.sub_cond(None, [0], L0, 16) is None and sampler.fit_cond(None, L0, 32) is None
    # shards
    kw = sampler.shard_cond_kwargs({"sample_bb": fl, "sample_seq": False, "aa_allowed": al, "start": st, "t_start": 0.5, "buckets": False}, 1, 3, B)
    assert torch.equal(kw["sample_bb"], fl[1:3]) and kw["sample_seq"] is False and torch.equal(kw["aa_allowed"], al[1:3])
    assert torch.equal(kw["start"]["trans"], st["trans"][1:3]) and kw["start"]["seqs"].shape == (2, L0) and kw["t_start"] == 0.5
    per_res = torch.ones(L0, 20, dtype=torch.bool)
    kw = sampler.shard_cond_kwargs({"aa_allowed": per_res, "start": "native"}, 1, 3, B)
    assert kw["aa_allowed"] is per_res and kw["start"] == "native"


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def _header_fields(struct):
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
            fields += [(n.strip(), {"int": C.c_int, "float": C.c_float}[ctype]) for n in names.split(",")]
    return fields


def test_struct_layout_and_header_order():
    cls = _capi.SamplerCondArgs
    assert [(n, t) for n, t in cls._fields_] == _header_fields("pf_sampler_cond_args")
    assert C.sizeof(cls) == 7 * 8 and cls.partial.offset == 0 and cls.start_rot.offset == 8 and cls.aa_allowed.offset == 48
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    order = [text.index(s) for s in ("} pf_sampler_args;", "int pf_sampler_init(", "int pf_sampler_step(", "} pf_sampler_cond_args;",
                                      "int pf_sampler_init_cond(", "int pf_sampler_step_cond(", "int pf_so3_geodesic(")]
    assert order == sorted(order)
    syms = _capi.EXPORTED_SYMBOLS
    k = syms.index("pf_sampler_step")
    assert syms[k + 1:k + 3] == ("pf_sampler_init_cond", "pf_sampler_step_cond") and syms[k - 1] == "pf_sampler_init"


def test_library_exports_and_checks_arguments():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_sampler_init_cond(None, None, None, None, None, None, None) == -1
    assert lib.pf_sampler_step_cond(None, None, None) == -1
    a, c = _capi.SamplerArgs(), _capi.SamplerCondArgs()
    assert lib.pf_sampler_init_cond(C.byref(a), C.byref(c), None, None, None, None, None) == -1       # incomplete sampler args
    assert lib.pf_sampler_step_cond(C.byref(a), C.byref(c), None) == -1
    # complete sampler args (dummy non-NULL addresses: the check returns before anything is launched or read) with a partial start
    # that lacks one of its four tensors
    for name, typ in _capi.SamplerArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, 64)
    a.num_steps, a.B, a.L = 3, 1, 16
    for missing in ("start_rot", "start_trans", "start_ang", "start_seq"):
        c = _capi.SamplerCondArgs()
        c.partial = 1
        for name in ("start_rot", "start_trans", "start_ang", "start_seq"):
            setattr(c, name, None if name == missing else 64)
        assert lib.pf_sampler_init_cond(C.byref(a), C.byref(c), 64, 64, 64, 64, None) == -1, missing
        assert lib.pf_sampler_step_cond(C.byref(a), C.byref(c), None) == -1, missing
    c = _capi.SamplerCondArgs()
    assert lib.pf_sampler_init_cond(C.byref(a), C.byref(c), 64, 64, 64, None, None) == -1              # the noise pointers, as pf_sampler_init


def test_sample_signature_has_the_new_keywords():
    import inspect
    p = inspect.signature(flow_model.FlowModel._sample_impl).parameters
    for k in ("t_start", "ts", "start", "aa_allowed"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None
    assert inspect.signature(sampler.DeviceSampler.__init__).parameters["cond"].default is False
