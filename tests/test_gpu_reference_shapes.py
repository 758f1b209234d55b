"""The production-shape kernel plans against arrays recorded from the REFERENCE (run on a real MI355X).

Golden F2 - F6 stop at L = 32, where DenoiseEngine runs none of the forms it runs for 64 <= L <= 256 (pair values and the two-kernel
attention, the fragment-ordered pair tensor, the hand-scheduled EdgeTransition streams v5 / v5h, the projection inside the score
kernel with folded keys, the k-fragment scratch, the f16 operand planes) and the training step none of its large-shape forms.  The
fixtures read here were recorded from the reference at those lengths (tests/ref_shapes.py, tests/golden/make_golden_f17.py, _f18,
_f19): F17 one denoise step per plan class, F18 a 3-step sample() with recorded RNG, F19 one training step.  Node and edge
embeddings come from the CPU restatement's encode() at test time (tests/test_oracle_golden.py pins it to the reference's at these
shapes, exactly).  Every case first asserts, against a LITERAL table, that the engine ran the plan the case is there for: a changed
threshold fails the case instead of silently moving it to another form.  Every bar is the one an existing test holds for the same
quantity at L <= 32.
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from oracle import pepflow_oracle as O  # noqa: E402  (checker only)
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, backward  # noqa: E402
import gpu_util as G  # noqa: E402
import ref_shapes as S  # noqa: E402
from test_gpu_parity import REL, F16_LOGIT_TOL  # noqa: E402
from test_gpu_train_shapes import Forms, _RecordCalls, _library_forms  # noqa: E402

SET = "set"                # a device buffer is allocated
# L -> what DenoiseEngine.__init__ must have decided; True / False / None are compared with `is`
PLAN_FP32 = {
    64: dict(fused_pair=True, z_frag=True, et_v5=True, fused_proj=True, k_fold=True, att_vt32=SET, pair_dz=SET,
             k_frag_s=None, k_frag=None, attn_p=None, z16=False, att_planes=False, et_v5h=False),
    128: dict(z_frag=True, et_v5=True, fused_proj=True, k_fold=True, k_frag_s=SET, att_vt32=SET, pair_dz=SET,
              fused_pair=False, attn_p=SET, k_frag=None, z16=False, att_planes=False, et_v5h=False),
    68: dict(fused_proj=True, k_fold=True, k_frag_s=SET, pair_dz=SET, z_frag=False, et_v5=False, et_v4=True, row_on=None,
             fused_pair=False, attn_p=SET, k_frag=None, z16=False),
    70: dict(fused_proj=False, k_fold=False, k_frag=None, z_frag=False, et_v5=False, et_v4=True, pair_dz=SET, fused_pair=False,
             attn_p=SET, k_frag_s=None, att_vt32=None, row_on=None, z16=False),
    144: dict(fused_proj=False, k_frag=SET, z_frag=True, et_v5=True, fused_pair=False, attn_p=SET, pair_dz=SET, k_frag_s=None,
              att_vt32=None, z16=False),
    272: dict(pair_dz=None, pair_dz0=None, z_frag=False, et_v5=False, fused_proj=False, fused_pair=False, k_frag=None,
              k_frag_s=None, att_vt32=None, z16=False),
}
PLAN_F16 = {
    64: dict(z16=True, att_planes=True, fused_pair=True, et_v5h=True, z_frag=True, fused_proj=True, att_qk=None, att_vt=None,
             attn_p=None, et_v5=False, k_fold=False),
    128: dict(z16=True, att_planes=True, fused_pair=True, et_v5h=True, z_frag=True, fused_proj=True, att_qk=None, att_vt=None,
              attn_p=None, et_v5=False, k_fold=False),
    144: dict(z16=True, att_planes=True, fused_pair=True, et_v5h=True, z_frag=True, fused_proj=False, att_qk=SET, att_vt=SET,
              attn_p=None, et_v5=False),
    272: dict(z16=False, att_planes=False, fused_pair=False, et_v5h=False, z_frag=False, fused_proj=False, att_qk=None,
              att_vt=None, pair_dz=None, et_v5=False),
}
# the training step's forms (tests/test_gpu_train_shapes.py: Forms) at the F19 shapes; (2, 64) has exactly 8192 pairs, the first size
# of the split-precision and wide products
TRAIN_FORMS = {64: Forms(fused_node=True, two_kernel_attn=True, virtual_x=True, tn_sum2=False, split_wide=True),
               128: Forms(fused_node=True, two_kernel_attn=True, virtual_x=True, tn_sum2=False, split_wide=True)}


def assert_plan(eng, B, L, precision, table):
    assert (eng.B, eng.L, eng.precision) == (B, L, precision), (eng.B, eng.L, eng.precision)
    for name, want in table[L].items():
        got = getattr(eng, name)
        ok = torch.is_tensor(got) if want is SET else got is want
        assert ok, f"L = {L}, {precision}: engine.{name} is {'a buffer' if torch.is_tensor(got) else got!r}, the case is there for {want!r}"


def cu(t):
    return t.to(G.dev()).contiguous()


def _ids(shapes):
    return [f"{B}x{L}" for B, L, _ in shapes]


_PARTS = {}


def _parts(golden_dir, stem):
    if stem not in _PARTS:
        _PARTS[stem] = S.load_parts(golden_dir, stem)
    return _PARTS[stem]


_ENC = {}


def _encoded(sd, stem, batch):
    """Node and edge embedding of a fixture's batch from the restatement's encode(), once per process."""
    if stem not in _ENC:
        _ENC[stem] = O.encode(sd, batch)
    return _ENC[stem]


def _new_model(sd, train=False, engine_options=None):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(sd, strict=True)
    if engine_options:
        m.ga_encoder.engine_options = engine_options
    m = m.to(G.dev())
    return m.train() if train else m.eval()


@pytest.fixture(scope="module")
def model(seeded_sd):
    return _new_model(seeded_sd)


def _step(m, f, b, node, edge):
    out = m.ga_encoder(cu(f["t"]), cu(f["R_t"]), cu(f["x_t"]), cu(f["ang_t"]), cu(f["seq_t"]), cu(node), cu(edge),
                       cu(b["generate_mask"].long()), cu(b["res_mask"].long()))
    G.sync()
    return [t.cpu() for t in out], m.ga_encoder.last_engine


def _node_state_per_block(eng):
    """The bound step once more, launch by launch (DenoiseEngine.run's serial order): the node state in front of the attention of
    blocks 1 .. 5 and after the last launch = after blocks 0 .. 5."""
    states, n_attn = [], 0
    for entry in eng.plan:
        fn, args, name = entry[0], entry[1], entry[2]
        if fn is None:
            continue
        if name == "pf_ipa_attn_fwd":
            if n_attn:
                states.append(eng.s.clone())
            n_attn += 1
        st = _capi.stream_ptr()
        _capi.check(fn(*args, st) if isinstance(args, tuple) else fn(args, st), name)
    states.append(eng.s.clone())
    G.sync()
    assert n_attn == O.N_BLOCKS and len(states) == O.N_BLOCKS
    return [s.cpu() for s in states]


def _close(a, b, rel, what):
    print(f"    {what}: max|a-b|/max|b| = {G.rel_err(a, b):.3e} (bar {rel:.1e})")
    G.assert_close(a, b, rel, what)


def _step_fp32(golden_dir, seeded_sd, model, B, L):
    """One denoise step in the fp32 mode against the reference's (golden F17), per plan class: outputs, the node state after every
    block, and the pair state after block 4 where the engine keeps it as fp32 [B, L, L, 64] rows -- with the bars test_ga_encoder_step
    holds for F2.

    The pair state: with the fragment-ordered pair tensor (L = 64, 128, 144) no buffer holds z in row order, so it is not compared
    there.  At L = 68 and 70 the plan does not store the last EdgeTransition's z' at all (nobody reads it); there a second engine
    with options={'et_last_store': True} runs the same step, must return the same bits, and its stored rows are compared."""
    stem = "f17_" + S.tag(B, L)
    f = _parts(golden_dir, stem)
    b, rows = S.batch_of(f), f["rows"]
    node, edge = _encoded(seeded_sd, stem, b)[4:]
    (R, x, ang, logits), eng = _step(model, f, b, node, edge)
    assert_plan(eng, B, L, "fp32", PLAN_FP32)
    valid = b["res_mask"]
    vflat = valid.reshape(-1)
    _close(eng.s.cpu()[vflat], f["s_blk_5"].reshape(-1, 128)[vflat], REL, "node state after block 5")
    for blk, s in enumerate(_node_state_per_block(eng)):
        _close(s[vflat], f[f"s_blk_{blk}"].reshape(-1, 128)[vflat], REL, f"node state after block {blk}")
    em = S.take_rows((valid[:, None, :] & valid[:, :, None])[..., None].expand(B, L, L, 64), rows)
    if not eng.z_frag:
        zeng = eng
        if eng.pair_dz is not None:
            (R2, x2, ang2, logits2), zeng = _step(_new_model(seeded_sd, engine_options={"et_last_store": True}), f, b, node, edge)
            assert_plan(zeng, B, L, "fp32", PLAN_FP32)
            assert all(torch.equal(p, q) for p, q in ((R, R2), (x, x2), (ang, ang2), (logits, logits2)))
        assert zeng.zbuf.dtype == torch.float32 and tuple(zeng.zbuf.shape) == (B, L, L, 64)
        _close(S.take_rows(zeng.zbuf.cpu(), rows)[em], f["z_blk_4_rows"][em], REL, "pair state after block 4")
    else:
        assert L in (64, 128, 144)
    _close(R[valid], f["out_R"][valid], REL, "pred rotmats")
    _close(x[valid], f["out_x"][valid], REL, "pred trans")
    _close(logits[valid], f["out_logits"][valid], REL, "seq logits")
    d = (ang[valid] - f["out_ang"][valid]).abs()
    assert torch.minimum(d, 2 * math.pi - d).max() < 2e-4, "angles"


def _step_f16(golden_dir, seeded_sd, model, B, L):
    """The same step in the f16 mode (f16 pair tensor and operand planes, pair aggregation inside the score kernel, the v5h
    EdgeTransition stream) against the reference at the project's f16 bars."""
    stem = "f17_" + S.tag(B, L)
    f = _parts(golden_dir, stem)
    b = S.batch_of(f)
    node, edge = _encoded(seeded_sd, stem, b)[4:]
    model.ga_encoder.set_precision("f16")
    try:
        (R, x, ang, logits), eng = _step(model, f, b, node, edge)
    finally:
        model.ga_encoder.set_precision("fp32")
    assert_plan(eng, B, L, "f16", PLAN_F16)
    valid = b["res_mask"]
    _close(R[valid], f["out_R"][valid], 1.2e-2, "pred rotmats")
    _close(x[valid], f["out_x"][valid], 3e-3, "pred trans")
    _close(logits[valid], f["out_logits"][valid], F16_LOGIT_TOL, "seq logits")
    d = (ang[valid] - f["out_ang"][valid]).abs()
    assert torch.minimum(d, 2 * math.pi - d).max() < 3e-2, "angles"


STEP_CASES = [("fp32",) + c for c in S.F17_SHAPES] + [("f16",) + c for c in S.F17_SHAPES if c[1] in (64, 128, 144, 272)]


@pytest.mark.parametrize("precision,B,L,lengths", STEP_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in STEP_CASES])
def test_step_vs_reference(golden_dir, seeded_sd, model, precision, B, L, lengths):
    """One denoise step against the reference's recorded step (golden F17) in the plan class of (L, precision): _step_fp32 / _step_f16."""
    (_step_fp32 if precision == "fp32" else _step_f16)(golden_dir, seeded_sd, model, B, L)


def _compare_trajectory(traj, f, ns):
    flips = sum((traj[i]["seqs"] != f[f"step{i}_seqs"]).sum().item() for i in range(ns))
    assert flips == 0, f"{flips} sequence flips"
    for i in range(ns):
        G.assert_close(traj[i]["rotmats"], f[f"step{i}_rotmats"], 2 * REL, f"step {i} rotmats")
        G.assert_close(traj[i]["trans"], f[f"step{i}_trans"], 2 * REL, f"step {i} trans")
        d = (traj[i]["angles"] - f[f"step{i}_angles"]).abs()
        assert torch.minimum(d, 2 * math.pi - d).max() < 1e-3, f"step {i} angles"
        assert torch.equal(traj[i]["seqs_simplex"], f[f"step{i}_seqs_simplex"])


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B,L,lengths", S.F18_SHAPES, ids=_ids(S.F18_SHAPES))
def test_trajectory_vs_reference(golden_dir, model, B, L, lengths, use_graph):
    """3-step free-running sample() with the reference's recorded noise (golden F18; every categorical decision of the reference
    has a relative margin >= 2e-3): no sequence flip, the continuous state as test_sample_trajectory_vs_reference holds it for F3.
    (1, 144) [137]: the batch cut to its 137 real residues, which sample() pads back to 144 itself, gives the same bits."""
    f = _parts(golden_dir, "f18_" + S.tag(B, L))
    ns = S.F18_STEPS
    assert f["margin"].item() >= S.F18_MIN_MARGIN
    b = {k: cu(v) for k, v in S.batch_of(f).items()}
    noise = {k: f[k] for k in S.NOISE_KEYS}
    traj = model.sample(b, num_steps=ns, noise=noise, use_graph=use_graph)
    assert len(traj) == ns and model.last_buckets is None
    assert_plan(model.ga_encoder.last_engine, B, L, "fp32", PLAN_FP32)
    _compare_trajectory(traj, f, ns)
    if (B, L) == (1, 144):
        L0 = lengths[0]
        cut = model.sample({k: v[:, :L0].contiguous() for k, v in b.items()}, num_steps=ns, use_graph=use_graph,
                           noise={k: (v[:, :, :L0] if k == "expo" else v[:, :L0]).contiguous() for k, v in noise.items()})
        assert_plan(model.ga_encoder.last_engine, B, L, "fp32", PLAN_FP32)
        for i in range(ns):
            for k in ("rotmats", "trans", "angles", "seqs", "seqs_simplex"):
                assert tuple(cut[i][k].shape[:2]) == (B, L0) and torch.equal(cut[i][k], traj[i][k][:, :L0]), (i, k)


@pytest.mark.parametrize("B,L,lengths", S.F19_SHAPES, ids=_ids(S.F19_SHAPES))
def test_training_step_vs_reference(golden_dir, seeded_sd, B, L, lengths, monkeypatch):
    """One eager training step against the reference's (golden F19): six losses at the bar of test_train_forward_losses_vs_reference,
    all 407 gradients through gpu_util.check_param_grads (3e-4 + 3 x the reference's own fp32 noise on that parameter), and the forms
    the step ran -- fused node track, two-kernel attention forward, virtual x, pair-sized products on the split-precision kernel and
    the wide gemm_tn -- from the names of its C-ABI calls."""
    import json
    f = dict(_parts(golden_dir, "f19_" + S.tag(B, L)))
    names = json.load(open(os.path.join(golden_dir, "f6_param_names.json")))
    f["_names"], f["_gradnorm"] = names, dict(zip(names, f["param_gradnorms"].tolist()))
    loose = [n for n, v in zip(names, f["param_fp32_noise"].tolist()) if v > S.F19_LOOSE_NOISE and not n.endswith("linear_b.bias")]
    assert len(loose) <= S.F19_MAX_LOOSE and S.F19_DISTCOEF in loose
    want = TRAIN_FORMS[L]
    assert _library_forms(B, L) == want, (_library_forms(B, L), want)
    assert B * L * L >= backward.SPLIT_MIN_ROWS == backward.TN_WIDE_MIN_ROWS == 8192

    virtual_seen, split_rows = set(), []
    et_forward, linear_split = backward.EdgeTransitionBlock.forward, backward._linear_split

    def forward(self, s, z):
        out = et_forward(self, s, z)
        virtual_seen.add(bool(self.virtual_x))
        return out

    def split(x, *a, **kw):
        split_rows.append(x.shape[0])
        return linear_split(x, *a, **kw)
    monkeypatch.setattr(backward.EdgeTransitionBlock, "forward", forward)
    monkeypatch.setattr(backward, "_linear_split", split)
    m = _new_model(seeded_sd, train=True)
    batch = {k: cu(v) for k, v in S.batch_of(f).items()}
    noise = {k: f[k] for k in S.TRAIN_NOISE_KEYS}
    with _RecordCalls() as calls:
        ld = m(batch, noise=noise)
        sum(O.LOSS_WEIGHTS[k] * v for k, v in ld.items()).backward()
        G.sync()
    ran = Forms(fused_node=calls["pf_node_tfmr_fwd"] > 0 and calls["pf_seq_attn_fwd"] == 0,
                two_kernel_attn=calls["pf_pair_bias_fwd"] > 0,
                virtual_x=calls["pf_gemm_tn_cat"] > 0,
                tn_sum2=calls["pf_gemm_tn_sum2"] > 0,
                split_wide=any(M == B * L * L for M in split_rows) and calls["pf_gemm_tn_wide"] > 1)
    assert ran == want, (ran, want, dict(calls))
    assert virtual_seen == {True} and min(split_rows) >= backward.SPLIT_MIN_ROWS, (virtual_seen, sorted(set(split_rows)))
    assert calls["pf_ipa_bwd_softmax"] == O.N_BLOCKS and calls["pf_et_bwd_chain"] == O.N_BLOCKS - 1, dict(calls)

    assert list(ld) == ["trans_loss", "rot_loss", "bb_atom_loss", "seqs_loss", "angle_loss", "torsion_loss"]
    for k, v in ld.items():
        ref = f["loss_" + k].item()
        assert abs(v.item() - ref) <= REL * abs(ref), (k, v.item(), ref)
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert len(grads) == 407
    worst = G.check_param_grads(grads, f, base=3e-4, k_noise=3.0)
    print(f"training step vs reference at ({B}, {L}): worst err/tol", worst)
