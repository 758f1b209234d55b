"""F14: the reference's structural-violation functions (vendored OpenFold, openfold/utils/loss.py: between_residue_bond_loss 712-868,
between_residue_clash_loss 871-1015, extreme_ca_ca_distance_violations 1235-1269) on seeded two-chain complexes: 40 + 12 residues,
NeRF backbones of ideal peptide geometry, side chains from the reference's own full_atom_reconstruction (models_con/torsion.py).

Cases (rows of every array):
  0  clean;
  1  every frame turned by 0.05 rad and moved by 0.1 A (per axis, Gaussian);          2  by 0.4 rad and 1 A;
  3  the peptide moved into the receptor (its centroid onto the receptor's; an open random chain, so few atoms meet);
  4  a numbering gap, a chain break, masked residues, missing side-chain atoms, a proline after a bond and one after the gap, two
     CYS with SG 2.05 A apart, two non-CYS slot-5 atoms 1 A apart;
  5  the two chains numbered alike (equal indices), the peptide inside the receptor, frames moved by 0.4 rad and 1 A;
  6  the peptide inside the receptor, frames moved by 0.4 rad and 1 A.
`batch_rows` names three rows that were also run as one batched call (B = 3): `batched_*`.

Recorded: the inputs in both residue-type numberings, the radius and C-N tables used, every output of the three functions, and the
smallest decision margin of any flag (float64, tests/violation_oracle.py).  The script reseeds until every flag array has between
5 % and 95 % set, case 0 has no bond violation and no margin is below 1e-3.
Build container only (needs the reference).  Data only.  Re-run: python tests/golden/make_golden_f14.py"""
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
from openfold.np import residue_constants as rc  # noqa: E402
from openfold.utils import loss as L  # noqa: E402
from models_con.torsion import full_atom_reconstruction  # noqa: E402
from pepflow.modules.common.geometry import construct_3d_basis  # noqa: E402
import dssp_build as DB  # noqa: E402
import violation_oracle as VO  # noqa: E402

DB.A_CACN = float(np.degrees(np.arccos(rc.between_res_cos_angles_ca_c_n[0])))      # ideal peptide geometry: 116.568, 121.352
DB.A_CNCA = float(np.degrees(np.arccos(rc.between_res_cos_angles_c_n_ca[0])))

PKG = "ACDEFGHIKLMNPQRSTVWY"                                                         # the package's numbering (AA)
PKG_TO_OF = np.array([rc.restypes.index(c) for c in PKG] + [20])
NA, NB = 40, 12
N = NA + NB
PRO, CYS, LEU, LYS = PKG.index("P"), PKG.index("C"), PKG.index("L"), PKG.index("K")

# tables in OpenFold's numbering, from its own names (loss.py:1127-1135: the first letter of the atom name is the element)
radius_of = np.zeros((21, 14), np.float32)
for t, c in enumerate(rc.restypes):
    for s, name in enumerate(rc.restype_name_to_atom14_names[rc.restype_1to3[c]]):
        if name:
            radius_of[t, s] = rc.van_der_waals_radius[name[0]]
radius_pkg = np.zeros((21, 14), np.float32)
radius_pkg[:20] = radius_of[PKG_TO_OF[:20]]


def rot_vec(v):
    return torch.from_numpy(np.stack([DB.rotation(x) for x in v]))


def complex_frames(rng):
    """two NeRF chains -> CA-centred frames R [N,3,3], t [N,3]; the peptide's centroid 14 A from the receptor's"""
    a, b = DB.random_chain(rng, NA)[:, :3], DB.random_chain(rng, NB)[:, :3]
    b = b @ DB.rotation(rng.standard_normal(3)).T
    d = rng.standard_normal(3)
    b = b - b[:, 1].mean(0) + a[:, 1].mean(0) + 14.0 * d / np.linalg.norm(d)
    bb = torch.from_numpy(np.concatenate([a, b]))
    return construct_3d_basis(bb[:, 1], bb[:, 2], bb[:, 0]), bb[:, 1]


def perturb(rng, R, t, rad, shift):
    v = rng.standard_normal((N, 3))
    v *= rad / np.linalg.norm(v, axis=1, keepdims=True)
    return rot_vec(v) @ R, t + torch.from_numpy(shift * rng.standard_normal((N, 3)))


def into_receptor(t):
    t = t.clone()
    t[NA:] += t[:NA].mean(0) - t[NA:].mean(0)
    return t


def atoms(R, t, ang, aa):
    return full_atom_reconstruction(R[None].float(), t[None].float(), ang[None].float(), torch.from_numpy(aa)[None])[0][0].numpy()


def make(seed):
    rng = np.random.default_rng(seed)
    R, t = complex_frames(rng)
    aa = rng.integers(0, 20, size=N)
    ang = torch.from_numpy(rng.uniform(0, 2 * np.pi, size=(N, 5)))
    index_plain = np.concatenate([np.arange(1, NA + 1), np.arange(NA + 3, NA + 3 + NB)]).astype(np.int32)
    S = 7
    pos = np.zeros((S, N, 14, 3), np.float32)
    aas = np.tile(aa, (S, 1))
    index = np.tile(index_plain, (S, 1))
    keep = np.ones((S, N, 14), bool)
    pos[0] = atoms(R, t, ang, aa)
    pos[1] = atoms(*perturb(rng, R, t, 0.05, 0.1), ang, aa)
    pos[2] = atoms(*perturb(rng, R, t, 0.4, 1.0), ang, aa)
    pos[3] = atoms(R, into_receptor(t), ang, aa)
    # case 4
    a4 = aa.copy()
    a4[10], a4[20] = PRO, PRO
    a4[5], a4[30] = CYS, CYS
    a4[8], a4[33] = LEU, LYS
    aas[4] = a4
    index[4, 20:NA] += 4                                    # the gap in front of residue 20 (a proline)
    index[4, NA:] = 200 + np.arange(NB)                     # the chain break
    p4 = atoms(R, t, ang, a4)
    u = rng.standard_normal((2, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p4[30, 5] = p4[5, 5] + 2.05 * u[0]
    p4[33, 5] = p4[8, 5] + 1.0 * u[1]
    pos[4] = p4
    keep[4, [14, 15, 44]] = False                           # masked residues
    keep[4, :, 4:] &= rng.random((N, 10)) > 0.1             # missing side-chain atoms
    keep[4, [5, 30, 8, 33], 5] = True
    # case 5
    index[5, NA:] = np.arange(1, NB + 1)
    Rp, tp = perturb(rng, R, into_receptor(t), 0.4, 1.0)
    pos[5] = atoms(Rp, tp, ang, aa)
    Rp, tp = perturb(rng, R, into_receptor(t), 0.4, 1.0)
    pos[6] = atoms(Rp, tp, ang, aa)

    aa_of = PKG_TO_OF[aas]
    exists = keep & (radius_of[aa_of] > 0)
    pos = pos * exists[..., None]                           # absent atoms at the origin, as padded inputs have them
    out = dict(pos=pos, atom_mask=exists, aa=aas.astype(np.int64), aa_openfold=aa_of.astype(np.int64), residue_index=index,
               radius_openfold=radius_of, radius=radius_pkg, pkg_to_openfold=PKG_TO_OF.astype(np.int64),
               pro=np.int64(PRO), pro_openfold=np.int64(rc.resname_to_idx["PRO"]),
               bond_length_c_n=np.array(rc.between_res_bond_length_c_n), bond_length_stddev_c_n=np.array(rc.between_res_bond_length_stddev_c_n),
               cos_angles_c_n_ca=np.array(rc.between_res_cos_angles_c_n_ca), cos_angles_ca_c_n=np.array(rc.between_res_cos_angles_ca_c_n),
               ca_ca=np.float64(rc.ca_ca), violation_tolerance_factor=np.float64(12.0), clash_overlap_tolerance=np.float64(1.5))

    def reference(rows):
        p, e = torch.from_numpy(pos[rows]), torch.from_numpy(exists[rows]).float()
        idx, t_of = torch.from_numpy(index[rows]).long(), torch.from_numpy(aa_of[rows]).long()
        bond = L.between_residue_bond_loss(p, e, idx, t_of, tolerance_factor_soft=12.0, tolerance_factor_hard=12.0)
        clash = L.between_residue_clash_loss(p, e, e * torch.from_numpy(radius_of)[t_of], idx, overlap_tolerance_soft=1.5,
                                             overlap_tolerance_hard=1.5)
        ca = L.extreme_ca_ca_distance_violations(p, e, idx)
        r = {"bond_" + k: v.numpy() for k, v in bond.items()}
        r.update({"clash_" + k: v.numpy() for k, v in clash.items()})
        r["extreme_ca_ca"] = ca.numpy()
        return r

    per = [reference(s) for s in range(S)]
    for k in per[0]:
        out["ref_" + k] = np.stack([r[k] for r in per])
    rows = np.array([0, 1, 3])
    out["batch_rows"] = rows
    for k, v in reference(rows).items():
        out["batched_" + k] = v

    # margins and the flags that the reference gives only as a mean (CA-CA), float64
    margin, brk, same = np.inf, [], True
    for s in range(S):
        o = VO.violations(pos[s], exists[s], aas[s], index[s], radius_pkg, PRO)
        same = same and np.array_equal(o["clash_atom"], per[s]["clash_per_atom_clash_mask"] > 0)
        same = same and np.array_equal(o["connection_violation"], per[s]["bond_per_residue_violation_mask"] > 0)
        margin = min(margin, o["clash_atom_margin"].min(), o["connection_margin"].min(), o["ca_ca_margin"].min())
        brk.append(o["ca_ca_break"])
    assert same or margin < 1e-3, "the float64 restatement and the reference disagree on a flag that is not near its threshold"
    out["ca_ca_break"] = np.stack(brk)
    out["min_margin"] = np.float64(margin)
    fractions = {k: float(np.mean(out[k] > 0)) for k in ("ref_clash_per_atom_clash_mask", "ref_bond_per_residue_violation_mask", "ca_ca_break")}
    ok = (all(0.05 <= f <= 0.95 for f in fractions.values()) and not out["ref_bond_per_residue_violation_mask"][0].any()
          and margin >= 1e-3)
    return ok, out, fractions


seed = 1400
while True:
    seed += 1
    ok, out, fractions = make(seed)
    print("seed", seed, fractions, "case 0 bond violations", int(out["ref_bond_per_residue_violation_mask"][0].sum()),
          "min margin", float(out["min_margin"]), "ok" if ok else "reseed")
    if ok:
        break
out["seed"] = np.int64(seed)
np.savez_compressed(os.path.join(HERE, "f14_violations.npz"), **out)
print("f14:", {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape})
