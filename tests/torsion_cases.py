"""Structures for the torsion tests, shared by the CPU tests (which run them through the oracle) and the GPU tests (through the
kernels): residues rebuilt from chosen chi angles by the float64 restatement of the full-atom reconstruction, NeRF backbones with
chain breaks, and the small constructed cases with known answers."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dssp_build as DB  # noqa: E402
from oracle import pepflow_oracle as O  # noqa: E402
from pepflowww_amd import geometry  # noqa: E402
from pepflowww_amd.preprocess import _tables, residue_type  # noqa: E402

_DATA = np.load(os.path.join(os.path.dirname(__file__), "..", "pepflowww_amd", "data", "rigid_groups.npz"))
TAB64 = {k: torch.from_numpy(_DATA[k]).double() if _DATA[k].dtype.kind == "f" else torch.from_numpy(_DATA[k])
         for k in ("rotation", "translation", "atom14_group", "atom14_position", "frames")}
HEAVY_MASK = _DATA["heavyatom_mask"][:21].copy()            # [21,15]
CHI = geometry.chi_atom_table().numpy()
PERIODIC = geometry.pi_periodic_table().numpy()
SWAP = geometry.swap_table().numpy()
GLY, ASP, LEU, LYS, PHE = (residue_type(n) for n in ("GLY", "ASP", "LEU", "LYS", "PHE"))
NAMES = _tables()["atom_names"]


def frames_of(bb):
    """N, CA, C [n,>=3,3] -> (R [n,3,3], t [n,3]) of the package's backbone frame: origin CA, x along C - CA, N in the xy half-plane y > 0"""
    n, ca, c = bb[:, 0], bb[:, 1], bb[:, 2]
    e1 = (c - ca) / np.linalg.norm(c - ca, axis=-1, keepdims=True)
    v = n - ca
    v = v - (v * e1).sum(-1, keepdims=True) * e1
    e2 = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return np.stack([e1, e2, np.cross(e1, e2)], -1), ca


def rebuild(R, t, angles, aa):
    """float64 full-atom reconstruction of residues of types aa (0..19) -> pos14 [n,14,3] float64"""
    f = lambda x: torch.from_numpy(np.asarray(x, np.float64))[None]  # noqa: E731
    return O.full_atom(f(R), f(t), f(angles), torch.from_numpy(np.asarray(aa, np.int64))[None], TAB64)[0][0].numpy()


def residues(aa, angles, R=None, t=None, A=15):
    """residues of types aa [n] (0..19) with model angles [n,5] (psi, chi1-4) in frames (R, t) (default: the identity at the origin)
    -> pos [n,A,3] fp32, mask [n,A] bool (the type's heavy atoms, no OXT)"""
    aa = np.asarray(aa, np.int64)
    n = len(aa)
    R = np.tile(np.eye(3), (n, 1, 1)) if R is None else R
    t = np.zeros((n, 3)) if t is None else t
    pos = np.zeros((n, A, 3), np.float32)
    pos[:, :14] = rebuild(R, t, angles, aa)
    mask = np.zeros((n, A), bool)
    mask[:, :14] = HEAVY_MASK[aa, :14]
    return pos, mask


def make_batch(rng, B, N, scale=60.0, A=15, breaks=(), aa=None):
    """B structures of N residues within +-scale: NeRF backbone segments of up to 20 residues placed at random, a new segment also at
    every position of `breaks`; every residue rebuilt in the frame of its N, CA, C from random angles, so each chi is that of ideal
    geometry (well conditioned); types `aa`, by default 0..21 and a -1 (types outside 0..19 are built as glycine and keep N, CA, C, O); masks with
    holes; the last sample all masked.  -> pos [B,N,A,3] fp32, mask [B,N,A], aa [B,N], residue_index [B,N] int32 (growing by 1 inside a
    segment and by 2, 5 or -3 across segments)"""
    pos = np.zeros((B, N, A, 3), np.float32)
    mask = np.zeros((B, N, A), bool)
    if aa is None:
        aa = rng.integers(0, 22, size=(B, N)).astype(np.int64)
        aa[0, N // 2] = -1
    index = np.zeros((B, N), np.int32)
    for b in range(B):
        k, idx = 0, 0
        while k < N:
            n = int(min(N - k, rng.integers(1, 21)))
            cut = [c for c in breaks if k < c < k + n]
            if cut:
                n = min(cut) - k
            seg = DB.random_chain(rng, n) @ DB.rotation(rng.standard_normal(3) * 2.0).T
            seg = seg - seg.mean((0, 1)) + rng.uniform(-(scale - 45.0), scale - 45.0, 3)
            R, t = frames_of(seg)
            build = np.where((aa[b, k:k + n] >= 0) & (aa[b, k:k + n] < 20), aa[b, k:k + n], GLY)
            p, m = residues(build, rng.uniform(0, 2 * np.pi, (n, 5)), R, t, A)
            unk = build != aa[b, k:k + n]
            m[unk] = False
            m[unk, :4] = True
            pos[b, k:k + n], mask[b, k:k + n] = p, m
            index[b, k:k + n] = idx + np.arange(n)
            idx += n - 1 + int(rng.choice([2, 5, -3]))
            k += n
        if A > 14:
            pos[b, :, 14:] = pos[b, :, 1:2] + rng.standard_normal((N, A - 14, 3)).astype(np.float32)
            mask[b, :, 14:] = rng.random((N, A - 14)) > 0.5
    mask &= (rng.random((B, N, A)) > 0.06) & (rng.random((B, N, 1)) > 0.05)
    mask[B - 1] = False
    assert np.abs(pos).max() <= scale
    return pos, mask, aa, index


def four_atoms(deg):
    """one glycine whose N, CA, C, O have the dihedral `deg` exactly in float64: CA at the origin, C on x, N and O one unit off the axis"""
    pos, mask = np.zeros((1, 15, 3)), np.zeros((1, 15), bool)
    a = np.radians(deg)
    pos[0, 0] = [-0.5, 1.0, 0.0]
    pos[0, 2] = [1.5, 0.0, 0.0]
    pos[0, 3] = [2.0, np.cos(a), np.sin(a)]
    mask[0, :4] = True
    return pos.astype(np.float32), mask, np.array([GLY], np.int64)


def collinear():
    """one glycine with N, CA, C on the x axis (psi_o, and nothing else, has its four atoms)"""
    pos, mask, aa = four_atoms(60.0)
    pos[0, 0] = [-1.0, 0.0, 0.0]
    return pos, mask, aa


def chain4(rng):
    """four alanines on one NeRF backbone, every atom present -> pos [4,15,3], mask, aa"""
    R, t = frames_of(DB.random_chain(rng, 4))
    pos, mask = residues(np.zeros(4, np.int64), rng.uniform(0, 2 * np.pi, (4, 5)), R, t)
    return pos, mask, np.zeros(4, np.int64)


CHI_ERRORS = (10.0, 19.0, 21.0, 170.0, 180.0)


def chi_error_pair(aa, chi_slot, base_deg=37.0):
    """five residues of type aa whose chi `chi_slot` (1..4) differs between x and y by CHI_ERRORS degrees, every other angle equal
    -> (pos_x, mask, aa [5]), (pos_y, mask, aa)"""
    n = len(CHI_ERRORS)
    ang = np.radians(np.tile([50.0, 295.0, 170.0, 65.0, 185.0], (n, 1)))
    ang[:, chi_slot] = np.radians(base_deg)
    ang_y = ang.copy()
    ang_y[:, chi_slot] += np.radians(CHI_ERRORS)
    t = np.arange(n)[:, None] * np.array([3.8, 0.0, 0.0])
    types = np.full(n, aa, np.int64)
    px, m = residues(types, ang, t=t)
    py, _ = residues(types, ang_y, t=t)
    return (px, m, types), (py, m.copy(), types.copy())


def exchanged(aa, names):
    """one residue of type aa, and the same with the coordinates of the atom pairs `names` exchanged, in another frame"""
    ang = np.radians([[50.0, 295.0, 40.0, 65.0, 185.0]])
    types = np.array([aa], np.int64)
    px, m = residues(types, ang)
    R = DB.rotation(np.array([0.3, -1.1, 0.7]))[None]
    py, _ = residues(types, ang, R=R, t=np.array([[5.0, -3.0, 2.0]]))
    for u, v in names:
        i, j = NAMES[aa].index(u), NAMES[aa].index(v)
        py[0, [i, j]] = py[0, [j, i]]
    return (px, m, types), (py, m.copy(), types.copy())
