"""One denoise step of DenoiseEngine (fp32 mode) against the float64 oracle, block by block and region by region (run on a real MI355X).

Every other forward test of the step compares whole tensors at 1e-4 against the oracle's fp32 run and, in the production plans, never
the pair tensor, the pair bias or the pair values.  Here the bound step is run launch by launch, in the serial order of
DenoiseEngine.run, and everything one block hands to the next is snapshot and compared with tests/step_oracle.py:
    after bind_context                  pair_bias0, pair_dz0 (where set)                      -> bias_0, dz_0
    after each block's last node_tfmr   s, rot, trans                                         -> s_b, R_b, x_b
    after each EdgeTransition           pair_bias, pair_dz (where set), zbuf (where stored)   -> bias_{b+1}, dz_{b+1}, z_b
    after the last launch               rot, trans, ang_raw % 2 pi, logits                    -> out_*
under err = max|got - t64| / max|t64| <= rel + 3 x the oracle's own fp32 noise, per tensor and per region (whole, each sample, each
sample's last 16 residues as rows / row band / column band, the launch's last rows % 4 and pairs % 64), at BOTH rel = block_oracle.REL
(1e-4, the parity bar) and rel = block_oracle.FWD_REL (2e-5, the bar of the training blocks' saved-activation forwards); with a noise
of 1e-7 .. 4.4e-6 the tight tolerance is 2.0e-5 .. 3.3e-5.  Each case is the smallest shape at which its plan class runs; the plan is
asserted against a literal table first, so a moved threshold fails the case instead of re-routing it.

Measured on an MI355X: worst err / tol 0.07 .. 0.17 at rel = 2e-5 (always a frame R_b, err 1.8e-6 .. 4.6e-6 against an oracle fp32
noise of 1.6e-6 .. 3.0e-6 there), 0.07 .. 0.11 on the pair tensors (a pair bias, err 1.7e-6 .. 3.0e-6), in every default plan and under
every forced option; DESIGN section 4 has the table.  The cases found nothing to fix.
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from oracle import pepflow_oracle as O  # noqa: E402  (checker only)
from pepflowww_amd import _capi  # noqa: E402
from pepflowww_amd.engine import DenoiseEngine, PackedWeights, z_from_frag  # noqa: E402
import gpu_util as G  # noqa: E402
import block_oracle as K  # noqa: E402
import step_oracle as S  # noqa: E402
from test_gpu_reference_shapes import PLAN_FP32, SET, assert_plan  # noqa: E402

# L -> what DenoiseEngine.__init__ must have decided.  64 .. 272: the table of test_gpu_reference_shapes.  23 and 48: below 64 there are
# no pair values, so no fused pair phase, no fragment-ordered pair tensor, no v5 stream and no projection inside; the EdgeTransition is the
# 32x32 kernel in row order; the last block's row_on list exists for whole 16-row groups only.
_BELOW_64 = dict(pair_dz=None, pair_dz0=None, fused_pair=False, attn_p=SET, et_v4=True, z_frag=False, et_v5=False, et_v5h=False,
                 fused_proj=False, k_fold=False, o_premul=True, k_frag=None, k_frag_s=None, att_vt32=None, att_planes=False, z16=False)
PLAN = {**PLAN_FP32, 23: dict(_BELOW_64, row_on=None), 48: dict(_BELOW_64, row_on=SET)}

# (option, forced value, case): the smallest L at which the option changes the plan
FORCED = [("et_v5", False, "64"), ("et_zfrag", False, "64"), ("fused_proj", False, "64"), ("fused_pair", False, "64"),
          ("fused_pair", True, "128"), ("k_fold", False, "128"), ("o_premul", False, "128"), ("k_frag", False, "144"),
          ("et_v4", False, "68"), ("et_last_store", True, "68")]
OUTPUTS = ("out_R", "out_x", S.ANGLE, "out_logits")


def cu(t):
    return t.to(G.dev()).contiguous()


@pytest.fixture(scope="module")
def weights(seeded_sd):
    return PackedWeights({k: cu(v) for k, v in seeded_sd.items()}, G.dev())


def _engine(weights, tr, options=None):
    c = tr["case"]
    eng = DenoiseEngine(weights, tr["B"], tr["L"], G.dev(), precision="fp32", options=options)
    eng.bind_context(cu(c["node"]), cu(c["edge"]), cu(c["batch"]["res_mask"]))
    eng.set_state(cu(c["t"]), cu(c["R_t"]), cu(c["x_t"]), cu(c["ang_t"]), cu(c["seq_t"]))
    return eng


def _et_stores(eng):
    """per EdgeTransition launch of the plan: does it store z'?  Read from the launch's own arguments."""
    return [bool(e[1]._obj.z_out) for e in eng.plan if e[2] == "pf_edge_transition_fwd"]


def _snapshots(eng):
    """The bound step launch by launch (DenoiseEngine.run's serial order) -> ({tensor name of step_oracle: device clone}, absent)."""
    B, L = eng.B, eng.L
    got = {"bias_0": eng.pair_bias0.permute(0, 2, 3, 1).contiguous()}
    if eng.pair_dz0 is not None:
        got["dz_0"] = eng.pair_dz0.clone()
    stores = _et_stores(eng)
    n_tfmr = n_et = 0
    for entry in eng.plan:
        fn, args, name = entry[0], entry[1], entry[2]
        if fn is None:
            continue
        st = _capi.stream_ptr()
        _capi.check(fn(*args, st) if isinstance(args, tuple) else fn(args, st), name)
        if name == "pf_node_tfmr_fwd":
            n_tfmr += 1
            if n_tfmr % 2 == 0:
                b = n_tfmr // 2 - 1
                got[f"s_{b}"], got[f"R_{b}"], got[f"x_{b}"] = eng.s.clone(), eng.rot.clone(), eng.trans.clone()
        elif name == "pf_edge_transition_fwd":
            b, n_et = n_et, n_et + 1
            assert n_tfmr == 2 * (b + 1)
            got[f"bias_{b + 1}"] = eng.pair_bias.permute(0, 2, 3, 1).contiguous()
            if eng.pair_dz is not None:
                got[f"dz_{b + 1}"] = eng.pair_dz.clone()
            if stores[b]:
                got[f"z_{b}"] = z_from_frag(eng.zbuf) if eng.z_frag else eng.zbuf.clone()
    G.sync()
    assert n_tfmr == 2 * O.N_BLOCKS and n_et == O.N_BLOCKS - 1 == len(stores)
    got["out_R"], got["out_x"], got["out_logits"] = eng.rot.clone(), eng.trans.clone(), eng.logits.clone()
    got[S.ANGLE] = eng.ang_raw % (2 * math.pi)
    # what this plan does not produce: pair values below 64 and beyond 256, the last z' where the launch does not store it
    drop_last = eng.pair_dz is not None and not eng.options.get("et_last_store", False)
    assert stores == [True] * (O.N_BLOCKS - 2) + [not drop_last], stores
    absent = [n for n in S.names() if n not in got]
    assert absent == ([] if eng.pair_dz is not None else [f"dz_{b}" for b in range(O.N_BLOCKS)]) + ([f"z_{O.N_BLOCKS - 2}"] if drop_last else []), absent
    return got, absent


def _form(eng):
    att = "projection inside" + (", keys folded" if eng.k_fold else "") if eng.fused_proj else "projection launch" + (", k fragments" if eng.k_frag is not None else "")
    att += ", shared k fragments" if eng.k_frag_s is not None else ""
    att += "; pair phase " + ("inside" if eng.fused_pair else ("in a second kernel" if eng.pair_dz is not None else "over z in the score kernel"))
    et = "v5 stream" if eng.et_v5 else ("32x32" if eng.et_v4 else "16x16")
    et += ", fragment order" if eng.z_frag else ", row order"
    return f"{att}; EdgeTransition {et}; o_premul {'on' if eng.o_premul else 'off'}"


def _check(tr, eng, got, absent, what):
    """Both rules, every figure printed before anything is asserted."""
    B, L, lengths, hole = S.CASES[tr["name"]]
    tight = S.compare(tr, got, K.FWD_REL, absent=absent, strict=False)
    loose = S.compare(tr, got, K.REL, absent=absent, strict=False)
    w, wl = tight["worst"], loose["worst"]
    wp = max((r for r in tight["rows"] if r[0].startswith(("z_", "bias_", "dz_"))), key=lambda r: r[2] / r[4])
    print(f"step forward vs float64 oracle: {what} ({B} x {L}, lengths {lengths}{', hole' if hole is not None else ''}): {_form(eng)}; "
          f"worst err/tol {w[0]:.3f} at {w[1]} / {w[2]} (err {w[3]:.2e}, oracle fp32 noise {w[4]:.2e}) at rel {K.FWD_REL:.0e}; "
          f"{wl[0]:.3f} at {wl[1]} / {wl[2]} at rel {K.REL:.0e}; pair tensors worst {wp[2] / wp[4]:.3f} at {wp[0]} / {wp[1]} (err {wp[2]:.2e}); {len(tight['rows'])} tensor regions, {len(absent)} tensors not produced")
    for b in tight["bad"][:12]:
        print("    outside the tight rule:", b)
    assert not loose["bad"], (what, K.REL, len(loose["bad"]), loose["bad"][:6])
    assert not tight["bad"], (what, K.FWD_REL, len(tight["bad"]), tight["bad"][:6])


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k].double() - b[k].double()).abs().max().item())


@pytest.mark.parametrize("name", list(S.CASES))
def test_step_forward_vs_float64_oracle(seeded_sd, weights, name):
    """Default plan, fp32 mode: the plan the case is there for, then every snapshot within both rules in every region.  Cases "64"
    and "144": a run() and a second launch-by-launch pass on the same bound engine give every snapshot bit for bit."""
    tr = S.truth(seeded_sd, name)
    eng = _engine(weights, tr)
    assert_plan(eng, tr["B"], tr["L"], "fp32", PLAN)
    got, absent = _snapshots(eng)
    _check(tr, eng, got, absent, name)
    if name in ("64", "144"):
        eng.run()
        G.sync()
        _same({k: got[k] for k in OUTPUTS}, {"out_R": eng.rot, "out_x": eng.trans, "out_logits": eng.logits,
                                             S.ANGLE: eng.ang_raw % (2 * math.pi)}, f"{name}: run() after the first pass")
        again, _ = _snapshots(eng)
        _same(got, again, f"{name}: second pass")


def _flag(eng, option):
    """the engine attribute an option flips, as a bool"""
    if option == "et_last_store":
        return _et_stores(eng)[-1]
    if option == "k_frag":
        return eng.k_frag is not None
    return bool(getattr(eng, {"et_zfrag": "z_frag"}.get(option, option)))


@pytest.mark.parametrize("option,value,name", FORCED, ids=[f"{o}={v}-{n}" for o, v, n in FORCED])
def test_forced_plan_option_vs_float64_oracle(seeded_sd, weights, option, value, name):
    """One forced option at the smallest L where it changes the plan: the attribute it flips differs from the default engine's, the
    same snapshots pass the same rules against the float64 truth (not form against form: a defect two forms share does not pass).
    et_last_store=True: z_4 is stored and compared, and the outputs equal the default engine's bit for bit."""
    tr = S.truth(seeded_sd, name)
    default = _engine(weights, tr)
    assert_plan(default, tr["B"], tr["L"], "fp32", PLAN)
    eng = _engine(weights, tr, options={option: value})
    assert (eng.B, eng.L, eng.precision) == (tr["B"], tr["L"], "fp32")
    assert _flag(eng, option) is value and _flag(default, option) is (not value), (option, value, _flag(eng, option), _flag(default, option))
    got, absent = _snapshots(eng)
    if option == "et_last_store":
        assert f"z_{O.N_BLOCKS - 2}" in got and not absent
        base, _ = _snapshots(default)
        _same({k: got[k] for k in OUTPUTS}, {k: base[k] for k in OUTPUTS}, "et_last_store against the default engine")
    _check(tr, eng, got, absent, f"{name}, {option}={value}")
