"""CPU checks of the fused optimizer layer: the float64 oracle (optim_oracle.py) against torch's CPU Adam / AdamW + clip_grad_norm_ on
the shared cases (this pins the oracle to the reference's semantics), the C ABI (struct layout against the header, exported symbols,
argument errors, ABI still 65, insertion points), the chunk-list builder, state_dict compatibility with torch.optim.Adam, the
refusals."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import optim_cases as OC  # noqa: E402
import optim_oracle as OO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, optim  # noqa: E402
from pepflowww_amd.optim import FusedAdam  # noqa: E402

EPS32 = 2.0 ** -24


@pytest.mark.parametrize("config", list(OC.CONFIGS))
def test_oracle_agrees_with_torch_adam_and_clip_grad_norm(config):
    """torch runs the block in fp32; one step from torch's own fp32 state differs from the float64 oracle by rounding only.  Bound: a
    moment is the sum of two rounded products of rounded factors and p subtracts a rounded quotient of them -- at most 16 roundings of
    2^-24 relative to the largest magnitude involved (for p: of the tensor or of lr, the size of an update).  A wrong formula (bias
    correction, L2 against decoupled decay, the clip coefficient, the NaN rule) misses this by orders of magnitude."""
    dev, norms = OC.reference_deviations(config)
    recs, _, _ = OC.run_torch(config)
    worst = 0.0
    for (k, name, q), (d, mag) in dev.items():
        bound = 16 * EPS32 * max(mag, OC.LR if q == "p" else 0.0)
        worst = max(worst, d / bound if bound else float(d > 0))
        assert d <= bound, (config, k, name, q, d, bound)
    print(f"{config}: worst torch-vs-oracle deviation = {worst:.3f} of the bound")
    if OC.CONFIGS[config]["max_norm"] is not None:
        for rec, (gn, _) in zip(recs, norms):
            assert abs(rec["grad_norm"] - gn) <= 8 * EPS32 * gn, (config, rec["step"], rec["grad_norm"], gn)
    assert [n for _, n in norms] == [sum(int(torch.isnan(g).sum()) for g in OC.make_grads(k) if g is not None) for k in range(len(OC.SCALES))]
    assert norms[1][1] > 0 and norms[0][1] == 0
    # the parameter without a gradient never moved and has no step
    i = OC.NAMES.index("no_grad")
    assert recs[-1]["after"][3][i] == 0 and np.array_equal(recs[-1]["after"][0][i], recs[0]["before"][0][i])


def test_cases_cover_the_clip_regimes():
    for config, want in (("adam_ref", {"inactive", "mild", "strong"}), ("adam_l2", {"inactive", "mild", "strong"})):
        seen = set()
        for k in range(len(OC.SCALES)):
            total, _, _ = OO.grad_norm([None if g is None else g.numpy() for g in OC.make_grads(k)])
            coef = OO.clip_coef(total, OC.CONFIGS[config]["max_norm"])
            seen.add("inactive" if coef == 1.0 else "mild" if coef > 0.5 else "strong")
        assert seen == want, (config, seen)
    assert OO.clip_coef(5.0, None) == 1.0 and OO.clip_coef(5.0, 0.0) == 1.0 and OO.clip_coef(5.0, -1.0) == 1.0


def test_oracle_skips_on_inf():
    p, g = [np.ones(3, np.float32)], [np.array([1.0, np.inf, np.nan], np.float32)]
    o = OO.step(p, g, [np.zeros(3)], [np.zeros(3)], [4], 1e-3, max_norm=1.0)
    assert o["skipped"] and o["steps"] == [4] and o["nan_count"] == 1 and np.array_equal(o["params"][0], p[0]) and o["grad_norm"] == np.inf


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_struct_layout_agrees_with_the_header():
    assert [(n, t) for n, t in _capi.OptimArgs._fields_] == header_fields("pf_optim_args")
    assert _capi.OptimArgs.n_chunks.offset + 4 <= C.sizeof(_capi.OptimArgs) and C.sizeof(_capi.OptimArgs) % 8 == 0
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} pf_optim_tensor;", text).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == list(optim.TENSOR_DTYPE.names)
    assert optim.TENSOR_DTYPE.itemsize == 48 and [optim.TENSOR_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 32, 36, 40, 44]


def test_header_constant_and_insertion_points():
    text = open(HEADER).read()
    assert f"#define PF_OPTIM_CHUNK {optim.CHUNK}" in text and optim.CHUNK % 1024 == 0
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("int pf_ipa_headw_bwd(") < text.index("} pf_optim_args;") < text.index("int pf_optim_step(") < text.index("} pf_superpose_args;")
    src = build.SOURCES
    assert src.index("et_bwd.hip") < src.index("optimizer.hip") < src.index("contacts.hip")
    syms = _capi.EXPORTED_SYMBOLS
    assert syms.index("pf_optim_step") + 1 == syms.index("pf_optim_work_bytes") < syms.index("pf_contacts_fwd")


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_optim_step(None, None) == -1
    assert lib.pf_optim_step(C.byref(_capi.OptimArgs()), None) == -1
    assert lib.pf_optim_work_bytes(1) == 64 + 16 and lib.pf_optim_work_bytes(2000) == 64 + 16 * 2000
    assert lib.pf_optim_work_bytes(0) == -1 and lib.pf_optim_work_bytes(-3) == -1 and lib.pf_optim_work_bytes(2 ** 31 - 1) == -1
    buf = (C.c_char * 64)()                             # host memory: a call that got as far as a launch would not return -1

    def args(**kw):
        a = _capi.OptimArgs()
        for name, typ in _capi.OptimArgs._fields_:
            setattr(a, name, C.addressof(buf) if typ is C.c_void_p else 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for bad in (dict(tensors=None), dict(hyper=None), dict(chunks=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(steps=None),
                dict(work=None), dict(result=None), dict(n_tensors=0), dict(n_groups=0), dict(n_chunks=0), dict(n_chunks=-1)):
        assert lib.pf_optim_step(C.byref(args(**bad)), None) == -1, bad


# ---- host layer --------------------------------------------------------------------------------------------------------------------

def test_chunk_list_covers_every_element_once():
    K = optim.CHUNK
    numels = [1, 3, K - 1, K, K + 1, 3 * K + 5]
    ch = optim.build_chunks(numels)
    assert ch.dtype == np.int32 and ch.shape == (1 + 1 + 1 + 1 + 2 + 4, 2)
    seen = [np.zeros(n, np.int32) for n in numels]
    for t, first in ch.tolist():
        assert first % K == 0 and 0 <= first < numels[t]                 # a chunk starts inside its tensor ...
        seen[t][first:min(first + K, numels[t])] += 1                    # ... and ends with it: none crosses into the next
    assert all((s == 1).all() for s in seen)
    assert ch[:, 0].tolist() == sorted(ch[:, 0].tolist())
    assert optim.build_chunks([0, 2]).tolist() == [[1, 0]]


def _cpu_pair(**kw):
    params = OC.make_params("cpu")
    return params, FusedAdam(params, lr=OC.LR, **kw)


def test_state_and_state_dict_have_torch_adams_layout():
    params, opt = _cpu_pair(max_grad_norm=100.0)
    ref_params = OC.make_params("cpu")
    ref = torch.optim.Adam(ref_params, lr=OC.LR)
    for p in ref_params:
        p.grad = torch.zeros_like(p)
    ref.step()
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert set(sd) == set(rsd) == {"state", "param_groups"}
    assert sd["param_groups"][0]["params"] == rsd["param_groups"][0]["params"] == list(range(len(params)))
    assert set(rsd["param_groups"][0]) <= set(sd["param_groups"][0])
    for k, s in rsd["state"].items():
        mine = sd["state"][k]
        assert set(mine) == set(s) == {"step", "exp_avg", "exp_avg_sq"}
        for key in s:
            assert mine[key].shape == s[key].shape and mine[key].dtype == s[key].dtype, (k, key)
    # state[p]: views of the two flat buffers and of the counters
    for i, p in enumerate(params):
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg"].untyped_storage().data_ptr() == opt.exp_avg.untyped_storage().data_ptr()
        assert st["exp_avg_sq"].untyped_storage().data_ptr() == opt.exp_avg_sq.untyped_storage().data_ptr()
        assert st["step"].untyped_storage().data_ptr() == opt.steps.untyped_storage().data_ptr() and st["exp_avg"].data_ptr() % 16 == 0
    # both directions: torch's state into FusedAdam (copied INTO the flat buffers), and back into a fresh torch Adam / AdamW
    opt.load_state_dict(rsd)
    assert opt.steps.tolist() == [1] * len(params) and opt.param_groups[0]["lr"] == OC.LR
    assert opt.state[params[3]]["exp_avg"].untyped_storage().data_ptr() == opt.exp_avg.untyped_storage().data_ptr()
    opt.state[params[2]]["exp_avg"].fill_(0.25)
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        back = cls(OC.make_params("cpu"), lr=1.0)
        back.load_state_dict(opt.state_dict())
        assert back.param_groups[0]["lr"] == OC.LR and float(back.state[back.param_groups[0]["params"][2]]["exp_avg"].max()) == 0.25
        assert all(float(s["step"]) == 1.0 for s in back.state.values())
        for p in back.param_groups[0]["params"]:
            p.grad = torch.ones_like(p)
        back.step()                                                      # torch accepts the groups as they came
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {}, "param_groups": [dict(rsd["param_groups"][0], params=[0, 1])]})


def test_schedulers_and_zero_grad_work_on_param_groups():
    params, opt = _cpu_pair()
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.8, patience=0)
    sched.step(1.0)
    sched.step(2.0)
    assert opt.param_groups[0]["lr"] == pytest.approx(OC.LR * 0.8)
    assert opt._hyper_rows()[1][0] == opt.param_groups[0]["lr"] and opt._hyper_rows()[0][0] == 0.0
    for cls, kw in ((torch.optim.lr_scheduler.MultiStepLR, dict(milestones=[1], gamma=0.5)), (torch.optim.lr_scheduler.ExponentialLR, dict(gamma=0.5))):
        cls(opt, **kw)
    params[0].grad = torch.ones_like(params[0])
    opt.zero_grad()
    assert params[0].grad is None


def test_refusals():
    params, opt = _cpu_pair()
    for p in params[:-1]:
        p.grad = torch.zeros_like(p)
    with pytest.raises(_capi.PepflowHipError):                           # no CPU fallback
        opt.step()
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(4, dtype=torch.float64, requires_grad=True)])
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(4, dtype=torch.bfloat16, requires_grad=True)])
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(4, 6).t().requires_grad_()])              # not contiguous
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            FusedAdam(OC.make_params("cpu"), **kw)
    with pytest.raises(ValueError):
        FusedAdam([])
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.zeros(2, requires_grad=True)]})
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError):
        opt.sync_groups()
    opt.param_groups[0]["amsgrad"] = False
    # gradients are validated when the pointer table is rebuilt: sparse, wrong dtype, non-contiguous, wrong shape
    e = torch.nn.Embedding(6, 4, sparse=True)
    e(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(ValueError, match="sparse"):
        FusedAdam(e.parameters()).sync_pointers()
    w = torch.zeros(4, 6, requires_grad=True)
    o2 = FusedAdam([w])
    for bad in (torch.zeros(4, 6, dtype=torch.float64), torch.zeros(6, 4).t(), torch.zeros(24)):
        with pytest.raises(ValueError):
            o2.sync_pointers([bad])
    from pepflowww_amd.train_step import GraphedTrainStep
    with pytest.raises(TypeError):
        GraphedTrainStep(torch.nn.Linear(2, 2), {}, {}, optimizer=torch.optim.Adam([w]))


def test_get_optimizer_mirrors_the_reference_factory():
    model = torch.nn.Linear(3, 2)
    a = optim.get_optimizer(types.SimpleNamespace(type="adam", lr=5e-4, weight_decay=0.0, beta1=0.9, beta2=0.999), model, max_grad_norm=100.0)
    g = a.param_groups[0]
    assert isinstance(a, FusedAdam) and (g["lr"], g["betas"], g["weight_decay"], g["decoupled_weight_decay"]) == (5e-4, (0.9, 0.999), 0.0, False)
    assert a.max_grad_norm == 100.0 and a._hyper_rows()[0][0] == 100.0
    w = optim.get_optimizer(types.SimpleNamespace(type="adamw", lr=1e-3, weight_decay=0.01), model)
    assert w.param_groups[0]["decoupled_weight_decay"] is True and w.param_groups[0]["betas"] == (0.9, 0.999) and w.max_grad_norm is None
    with pytest.raises(NotImplementedError):
        optim.get_optimizer(types.SimpleNamespace(type="sgd"), model)
