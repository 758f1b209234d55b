"""F17: one denoise step of the REFERENCE per plan class of the denoise engine (tests/ref_shapes.py: F17_SHAPES), with the
per-block node states and backbone updates through the same forward hooks as F2.  The pair-sized tensors (edge embedding,
pair state after block 4) are kept on a fixed set of query rows only.  Also records how far the CPU restatement
(oracle/pepflow_oracle.py, called as the tests call it) is from the reference on every stored tensor: `ref_vs_oracle_<name>`.
Needs the reference code base (imported through oracle/tools/ref_shim.py).  Re-run: python tests/golden/make_golden_f17.py"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from pepflowww_amd import synth  # noqa: E402
import ref_shapes as S  # noqa: E402
from oracle import pepflow_oracle as O  # noqa: E402

torch.set_num_threads(8)
model, cfg = ref_shim.build_reference_model()
sd = synth.seeded_state_dict()
model.load_state_dict(sd, strict=True)

from data import so3_utils  # noqa: E402
from openfold.utils import rigid_utils as ru  # noqa: E402

enc = model.ga_encoder
for B, L, lengths in S.F17_SHAPES:
    batch = S.f17_batch(B, L, lengths)
    rows = S.query_rows(L, lengths)
    resm = batch["res_mask"].long()
    genm = batch["generate_mask"].long()
    g = torch.Generator().manual_seed(S.f17_case_seed(L))
    with torch.no_grad():
        R1, x1, ang1, seq1, node, edge = model.encode(batch)
        t = torch.rand(B, 1, generator=g) * 0.9 + 0.05
        q = torch.randn(B, L, 4, generator=g)
        Rn = ru.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
        R_t = so3_utils.geodesic_t(t[..., None], R1, Rn)
        x_t = x1 + torch.randn(B, L, 3, generator=g)
        ang_t = torch.rand(B, L, 5, generator=g) * 2 * math.pi
        seq_t = torch.randint(0, 20, (B, L), generator=g)
        cap, hs = {}, []

        def hook(name):
            def fn(mod, inp, out):
                cap[name] = out.detach().clone()
            return fn
        for b in range(6):
            hs.append(enc.trunk[f"node_transition_{b}"].register_forward_hook(hook(f"trans_{b}")))
            hs.append(enc.trunk[f"bb_update_{b}"].register_forward_hook(hook(f"bbupd_{b}")))
        hs.append(enc.trunk["edge_transition_4"].register_forward_hook(hook("et_4")))
        pR, px, pang, plog = enc(t, R_t, x_t, ang_t, seq_t, node, edge, genm, resm)
        for h in hs:
            h.remove()
        em = (resm[:, None] * resm[:, :, None])[..., None]
        out = dict(out_R=pR, out_x=px, out_ang=pang, out_logits=plog)
        s_blk = {f"s_blk_{b}": cap[f"trans_{b}"] * resm[..., None] for b in range(6)}
        bbupd = {f"bbupd_{b}": cap[f"bbupd_{b}"] for b in range(6)}
        edge_rows = S.take_rows(edge, rows)
        z4_rows = S.take_rows(cap["et_4"] * em, rows)

        # the restatement on the same inputs, as the tests call it: its own encode(), then one step
        o_enc = O.encode(sd, batch)
        col = {}
        oR, ox, oang, olog = O.ga_encoder(sd, t, R_t, x_t, ang_t, seq_t, o_enc[4], o_enc[5], resm, collect=col)
    valid = batch["res_mask"]
    em_rows = S.take_rows(em.expand(B, L, L, 64), rows).bool()
    dist = {"enc_node": S.maxnorm(o_enc[4], node), "enc_edge": S.maxnorm(S.take_rows(o_enc[5], rows), edge_rows),
            "out_R": S.maxnorm(oR[valid], pR[valid]), "out_x": S.maxnorm(ox[valid], px[valid]),
            "out_logits": S.maxnorm(olog[valid], plog[valid]), "out_ang": S.circle(oang[valid], pang[valid]),
            "z_blk_4": S.maxnorm(S.take_rows(col["z_4"], rows)[em_rows], z4_rows[em_rows])}
    for b in range(6):
        dist[f"s_blk_{b}"] = S.maxnorm(col[f"s_{b}"][valid], s_blk[f"s_blk_{b}"][valid])
        dist[f"bbupd_{b}"] = S.maxnorm(col[f"upd_{b}"][valid], bbupd[f"bbupd_{b}"][valid])
    assert dist["enc_node"] <= 1e-6 and dist["enc_edge"] <= 1e-6, dist
    assert all(v <= S.ORACLE_CEILING for v in dist.values()), dist

    io = dict(t=t, R_t=R_t, x_t=x_t, ang_t=ang_t, seq_t=seq_t, rows=rows, enc_node=node, **out, **bbupd)
    io.update({"batch_" + k: v for k, v in batch.items()})
    io.update({"ref_vs_oracle_" + k: torch.tensor(v, dtype=torch.float64) for k, v in dist.items()})
    sizes = S.save_parts(HERE, "f17_" + S.tag(B, L), {"io": io, "s": s_blk, "edge": {"enc_edge_rows": edge_rows}, "z4": {"z_blk_4_rows": z4_rows}})
    print(f"F17 ({B}, {L}) {lengths}: " + ", ".join(f"{n} {sz / 1024:.1f} KiB" for n, sz in sizes))
    print("  ref_vs_oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in dist.items()))
print("done")
