"""F16: the reference's FlowModel.encode (flow_model.py:75-93) on the PDB-shaped inputs of tests/pocket_cases.py, seeded weights.

Recorded per case of pocket_cases.F16_CASES (frag19 (2, 19), frag33 (3, 33), wrap40 (2, 40), collinear (1, 19)): the batch and the
frames, node and pair embeddings of `encode` with both switches on.  For frag19 also the three other settings of
`model.sample_structure` / `model.sample_sequence`, set on the model as its config would (flow_model.py:69-70), and
NodeEmbedder.forward / EdgeEmbedder.forward called directly with `structure_mask=None` and with `sequence_mask=None` (asserted here to
equal the switch settings (0, 1) and (1, 0) bit for bit and stored once, as those).  For collinear
also `dihedral_from_four_points` on the two collinear point quadruples, and the outputs on the same batch with finite garbage in the
positions of masked side-chain atoms (asserted here to be the outputs without it, bit for bit, so they are not stored twice).

Two files of 0.6 and 0.7 MB, so that neither comes near F2's 0.9 MB and the full pair embeddings of all three samples of frag33 can
stay: f16_encode_inputs.npz (batches, frames, node embeddings, every array of frag19 and collinear) and f16_encode_edges.npz (the
pair embeddings of frag33 and wrap40); together 1.35 MB.
Build container only (needs the reference).  Data only.  Re-run: python tests/golden/make_golden_f16.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
import ref_shim  # noqa: E402
from pepflowww_amd import synth  # noqa: E402
import pocket_cases as P  # noqa: E402

torch.set_num_threads(8)
model, cfg = ref_shim.build_reference_model()
model.load_state_dict(synth.seeded_state_dict(), strict=True)
from pepflow.modules.common.geometry import dihedral_from_four_points  # noqa: E402

BATCH_KEYS = ("aa", "res_nb", "chain_nb", "pos_heavyatom", "mask_heavyatom", "generate_mask", "torsion_angle", "torsion_angle_mask", "res_mask")


def encode(batch, ss=True, sq=True):
    model.sample_structure, model.sample_sequence = ss, sq
    try:
        with torch.no_grad():
            return model.encode(batch)
    finally:
        model.sample_structure, model.sample_sequence = True, True


small, edges = {}, {}
for name in P.F16_CASES:
    full = P.make(name)
    batch = P.model_inputs(full)
    for k in BATCH_KEYS:
        small[f"{name}.batch_{k}"] = batch[k]
    R1, x1, ang1, seq1, node, edge = encode(batch)
    assert torch.equal(x1, batch["pos_heavyatom"][:, :, 1]) and torch.equal(seq1, batch["aa"]) and torch.equal(ang1, batch["torsion_angle"])
    assert all(torch.isfinite(t).all() for t in (R1, node, edge))
    small[f"{name}.R1"], small[f"{name}.node"] = R1, node
    if name in ("frag33", "wrap40"):
        edges[f"{name}.edge"] = edge
    else:
        small[f"{name}.edge"] = edge
    if name == "frag19":
        for ss, sq in P.SWITCHES[1:]:
            out = encode(batch, ss, sq)
            assert torch.equal(out[0], R1)
            small[f"{name}.node_ss{int(ss)}_sq{int(sq)}"], small[f"{name}.edge_ss{int(ss)}_sq{int(sq)}"] = out[4], out[5]
        ctx = batch["mask_heavyatom"][:, :, 1] & ~batch["generate_mask"]
        args = (batch["aa"], batch["res_nb"], batch["chain_nb"], batch["pos_heavyatom"], batch["mask_heavyatom"])
        # the stand-alone calls with one mask None are what encode computes with that switch off, bit for bit: stored once, under
        # the switch setting's name (tests compare the stand-alone calls of the port with those arrays)
        with torch.no_grad():
            for twin, kw in (("ss0_sq1", dict(structure_mask=None, sequence_mask=ctx)), ("ss1_sq0", dict(structure_mask=ctx, sequence_mask=None))):
                assert torch.equal(model.node_embedder(*args, **kw), small[f"{name}.node_{twin}"])
                assert torch.equal(model.edge_embedder(*args, **kw), small[f"{name}.edge_{twin}"])
    if name == "collinear":
        q = full["collinear_points"]
        small[f"{name}.points"] = q
        small[f"{name}.dihedrals"] = dihedral_from_four_points(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
        u1, sgn = P.dihedral_terms(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
        assert bool((u1 == 0).all()) and bool((sgn != 0).all()) and bool((small[f"{name}.dihedrals"] == 0).all()), (u1, sgn, small[f"{name}.dihedrals"])
        gb = P.model_inputs(P.make("collinear_garbage"))
        assert not torch.equal(gb["pos_heavyatom"], batch["pos_heavyatom"]) and gb["pos_heavyatom"].abs().max() > 500
        go = encode(gb)
        assert torch.equal(go[0], R1) and torch.equal(go[4], node) and torch.equal(go[5], edge), "garbage in masked side-chain slots moved the reference"

for fname, arrs in (("f16_encode_inputs.npz", small), ("f16_encode_edges.npz", edges)):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote {fname}: {size / 1024:.1f} KiB, {len(out)} arrays")
    assert size < 1024 * 1024, (fname, size)
