"""F15: the reference's lDDT (vendored OpenFold, openfold/utils/loss.py:382-458, `lddt` and `lddt_ca`) on the two-chain complexes of
F14 (f14_violations.npz: 40 + 12 residues, built by make_golden_f14.py from NeRF backbones and the reference's own
full_atom_reconstruction).  The reference structure y is F14's clean complex (row 0); the models x are, by row:
  0  the clean complex itself;
  1  every frame turned by 0.05 rad and moved by 0.1 A;             2  by 0.4 rad and 1 A;
  3  the peptide moved into the receptor;
  4  masked residues, missing side-chain atoms and a few residues of another type than the native's;
  5  the peptide inside the receptor, frames moved by 0.4 rad and 1 A.

Recorded: the inputs (pos, atom_mask, aa of x; y is row 0; `group`: the peptide), the mask of compared atoms that the reference was
given ([S, N * 14, 1]: both structures have the atom and, for side-chain slots, the residue types agree), `lddt` on the flattened 14-slot
atoms with per_residue True ([S, N * 14], one value per atom) and False ([S]), `lddt_ca` on the [N, 14] layout ([S, N] and [S]), and the
integer counts of tests/lddt_oracle.py for all atoms and for CA.  fp32 in, fp32 out, as the reference computes them.
Build container only (needs the reference).  Data only.  Re-run: python tests/golden/make_golden_f15.py"""
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
import ref_shim  # noqa: E402
ref_shim.install()
if "ml_collections" not in sys.modules:                 # loss.py names it only in annotations
    _m = types.ModuleType("ml_collections")
    _m.__spec__ = importlib.machinery.ModuleSpec("ml_collections", loader=None)
    _m.ConfigDict = dict
    sys.modules["ml_collections"] = _m
from openfold.utils import loss as L  # noqa: E402
import lddt_oracle as LO  # noqa: E402

f14 = np.load(os.path.join(HERE, "f14_violations.npz"))
ROWS = [0, 1, 2, 3, 4, 6]
S, N = len(ROWS), f14["pos"].shape[1]
pos, mask, aa = f14["pos"][ROWS].astype(np.float32), f14["atom_mask"][ROWS].astype(bool), f14["aa"][ROWS].astype(np.int64)
group = np.arange(N) >= 40

compared = np.stack([LO.compared_atoms(mask[s], aa[s], mask[0], aa[0], 0x3FFF) for s in range(S)])
x, y = torch.from_numpy(pos).reshape(S, N * 14, 3), torch.from_numpy(pos[:1]).expand(S, N, 14, 3).reshape(S, N * 14, 3)
m = torch.from_numpy(compared).float().reshape(S, N * 14, 1)
out = dict(pos=pos, atom_mask=mask, aa=aa, group=group, compared=compared, cutoff=np.float64(15.0),
           ref_lddt_atom=L.lddt(x, y, m, per_residue=True).numpy(), ref_lddt=L.lddt(x, y, m, per_residue=False).numpy())
x4, y4, m4 = x.reshape(S, N, 14, 3), y.reshape(S, N, 14, 3), m.reshape(S, N, 14)
out["ref_lddt_ca_residue"] = L.lddt_ca(x4, y4, m4, per_residue=True).numpy()
out["ref_lddt_ca"] = L.lddt_ca(x4, y4, m4, per_residue=False).numpy()

for tag, slots in (("", 0x3FFF), ("_ca", 0x2)):
    rows = [LO.lddt(pos[s], mask[s], aa[s], pos[0], mask[0], aa[0], slots, 15.0, group=group) for s in range(S)]
    for k in ("scored", "kept", "scored_cross", "kept_cross") + (("scored_atom", "kept_atom") if not tag else ()):
        out[k + tag] = np.stack([r[k] for r in rows]).astype(np.int32)

assert out["ref_lddt_atom"].shape == (S, N * 14) and out["ref_lddt_ca_residue"].shape == (S, N)
whole = LO.score(out["kept"].sum(1), out["scored"].sum(1))
print("lddt (reference)", out["ref_lddt"], "\nlddt (counts)   ", whole, "\nlddt_ca         ", out["ref_lddt_ca"])
assert np.abs(whole - out["ref_lddt"]).max() < 1e-3 and out["ref_lddt"][0] > 0.9999 and 0.2 < out["ref_lddt"][2] < 0.95
path = os.path.join(HERE, "f15_lddt.npz")
np.savez_compressed(path, **out)
print("f15:", {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
