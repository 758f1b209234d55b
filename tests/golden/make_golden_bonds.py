"""The reference's heavy-atom bond graph per residue type (pepflow/modules/protein/constants.py: restype_to_heavyatom_bond_matrix,
built from restype_to_bonded_atom_name_pairs), recorded as `bonds` [21,15,15] bool = (matrix != 0) in the reference's residue order
(AA 0..19 and UNK) and heavy-atom order, with the reference's residue and atom names beside it so that a test can check that both
orders are the package's.  geometry.bond_table states the same graph from chemistry; test_relax_cpu.py compares the two.  The
reference lists no bond for UNK (row 20 is empty here); the package's row 20 holds N-CA, CA-C and C=O.
Build container only (needs the reference).  Data only.  Re-run: python tests/golden/make_golden_bonds.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
import ref_shim  # noqa: E402
ref_shim.install()
from pepflow.modules.protein import constants as RC  # noqa: E402

types = [t for t in RC.AA if int(t) <= 20]
assert [int(t) for t in types] == list(range(21))
bonds = np.stack([(RC.restype_to_heavyatom_bond_matrix[t] != 0).numpy() for t in types])
names = np.array([[str(n) for n in RC.restype_to_heavyatom_names[t]] for t in types])
assert bonds.shape == (21, 15, 15) and names.shape == (21, 15) and np.array_equal(bonds, bonds.transpose(0, 2, 1))
path = os.path.join(HERE, "heavyatom_bonds.npz")
np.savez_compressed(path, bonds=bonds, atom_names=names, resnames=np.array([t.name for t in types]))
print("bonds per type:", dict(zip([t.name for t in types], (bonds.sum((1, 2)) // 2).tolist())), os.path.getsize(path), "bytes")
