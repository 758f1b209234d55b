"""Inputs of the cavity tests (test_cavity_cpu.py, test_gpu_cavity.py, test_gpu_design.py): the smallest shapes at which the kernels
of csrc/cavity.hip can still go wrong.  Not to be confused with pocket_cases.py (the receptor pockets of the sampler's tests).

Lattice cases: one atom per voxel of a boolean [vx, vy, vz] array, at voxel_origin + index (coordinates are multiples of 1/8 A below
64 A), packed 15 to a residue with the rest of the last residue masked; a constant radius table of 0.5 and a probe of 0.25 (R = 0.75), h
in {1, 0.5}: every coordinate, difference, squared distance and threshold is exact in fp32, so the kernel has to equal the float64
oracle exactly.  At h = 1 with grid points on the atoms an atom occupies its own point and no other (the next is 1 > 0.75 away): the
voxel array IS the occupancy, and the answers below are constructed by hand.

Each case is a dict: pos [N,15,3] float32, mask [N,15] bool, aa [N] int64, radius [21,15] float32, origin [3] float32, dims, h,
params (of the scan), exact (held to the float64 oracle; otherwise to the fp32-emulating one) and, where constructed, `answer`.
"""
import numpy as np

RADIUS_LATTICE = np.full((21, 15), 0.5, np.float32)
LATTICE_PARAMS = {"probe": 0.25, "r_lining": 1.5}


def atoms_of_voxels(vox, voxel_origin, masked_extra=3):
    """one atom per True voxel at voxel_origin + index, 15 to a residue; `masked_extra` residues of masked atoms lie in front, all
    at the middle of the voxel array: a kernel that ignores the mask occupies points there that it must not"""
    idx = np.argwhere(vox)
    xyz = idx.astype(np.float32) + np.asarray(voxel_origin, np.float32)
    n_res = (len(xyz) + 14) // 15 + masked_extra
    pos, mask = np.zeros((n_res, 15, 3), np.float32), np.zeros((n_res, 15), bool)
    flat_pos, flat_mask = pos[masked_extra:].reshape(-1, 3), mask[masked_extra:].reshape(-1)
    flat_pos[:len(xyz)] = xyz
    flat_mask[:len(xyz)] = True
    if masked_extra and vox.any():
        inside = np.asarray(voxel_origin, np.float32) + (np.asarray(vox.shape, np.float32) - 1) / 2       # a multiple of 1/2
        pos[:masked_extra, :] = inside
    aa = (np.arange(n_res) % 23 - 1).astype(np.int64)       # every type, and two outside 0..20 (they read row 20)
    return pos, mask, aa


def lattice_case(vox, dims, grid_shift=(0, 0, 0), origin=(0.0, 0.0, 0.0), h=1.0, answer=None, **params):
    """the voxel array put at grid index `grid_shift` of a grid with `origin`"""
    origin = np.asarray(origin, np.float32)
    pos, mask, aa = atoms_of_voxels(vox, origin + np.asarray(grid_shift, np.float32))
    return {"pos": pos, "mask": mask, "aa": aa, "radius": RADIUS_LATTICE, "origin": origin, "dims": tuple(dims), "h": h,
            "params": {**LATTICE_PARAMS, **params}, "exact": True, "answer": answer}


def box(outer, open_top=False):
    """a hollow box of wall thickness 1: [outer] voxels, the interior free; open_top removes the z-max wall's inner part"""
    v = np.ones(outer, bool)
    v[1:-1, 1:-1, 1:-1] = False
    if open_top:
        v[1:-1, 1:-1, -1] = False
    return v


def shell():
    """a closed hollow shell, 9 x 7 x 11 outside, in a 13 x 9 x 17 grid: one cavity, the 7 x 5 x 9 interior, buriedness 7 all over"""
    return lattice_case(box((9, 7, 11)), (13, 9, 17), grid_shift=(2, 1, 3), origin=(-2.0, -3.125, 1.5),
                        answer={"n_found": 1, "size": [7 * 5 * 9], "mean_buried": [7.0], "center": [[4.0, 0.875, 9.5]]})


def shell_half():
    """the same shell on a grid of h = 0.5 (27 x 19 x 35): an atom now occupies 19 points"""
    c = shell()
    c.update(dims=(27, 19, 35), h=0.5, answer={"n_found": 1})
    return c


def groove():
    """the shell without the inside of its z-max wall: a groove open on one face"""
    return lattice_case(box((9, 7, 11), open_top=True), (13, 9, 17), grid_shift=(2, 1, 3), origin=(-2.0, -3.125, 1.5),
                        answer={"n_found": 1})


def two_equal():
    """two closed boxes with 3 x 3 x 3 interiors, 7 free points apart along x, max_ray = 6 (n_axis 6, n_diag 3): two cavities of 27
    points -- the ranking's tie, the one at the lower x first; the gap between them is buried on one line at most"""
    v = np.zeros((17, 5, 5), bool)
    v[:5] = box((5, 5, 5))
    v[12:] = box((5, 5, 5))
    return lattice_case(v, (33, 20, 7), grid_shift=(9, 11, 1), origin=(3.0, -1.25, 0.375), max_ray=6.0,
                        answer={"n_found": 2, "size": [27, 27], "mean_buried": [7.0, 7.0],
                                "center": [[3.0 + 9 + 2, -1.25 + 11 + 2, 0.375 + 1 + 2], [3.0 + 9 + 14, -1.25 + 11 + 2, 0.375 + 1 + 2]]})


def _block_with(shape, chambers):
    v = np.ones(shape, bool)
    for sl in chambers:
        v[sl] = False
    return v


def diagonal_touch(connectivity):
    """a solid block with two 2 x 2 x 2 chambers that touch at one corner only: two cavities of 8 under 6-connectivity (a tie), one of
    16 under 26"""
    v = _block_with((8, 8, 8), [np.s_[2:4, 2:4, 2:4], np.s_[4:6, 4:6, 4:6]])
    answer = ({"n_found": 2, "size": [8, 8], "center": [[2.5, 2.5, 2.5], [4.5, 4.5, 4.5]]} if connectivity == 6 else
              {"n_found": 1, "size": [16], "center": [[3.5, 3.5, 3.5]]})
    return lattice_case(v, (8, 8, 8), connectivity=connectivity, answer=answer)


def serpentine():
    """a solid 40 x 9 x 9 block with a tunnel one point wide in the plane y = 4: runs along z at every odd x, joined at the ends in
    turn -- one component of 19 * 7 + 18 = 151 points that crosses some thirteen workgroups, with paths that long in the union-find"""
    v = np.ones((40, 9, 9), bool)
    for x in range(1, 38, 2):
        v[x, 4, 1:8] = False
    for j, x in enumerate(range(2, 37, 2)):
        v[x, 4, 7 if j % 2 == 0 else 1] = False
    return lattice_case(v, (40, 9, 9), answer={"n_found": 1, "size": [151], "mean_buried": [7.0]})


def many(max_cavities=3):
    """a solid 24 x 20 x 20 block (over 600 residues: beyond the 512 of the evaluation kernels) with six chambers of 3, 1, 2, 3, 5, 4 points
    along z, min_points = 1 and max_cavities = 3: six kept, the first three reported -- 5, 4, and of the two of 3 the first"""
    sizes, ch = [3, 1, 2, 3, 5, 4], []
    for j, s in enumerate(sizes):
        ch.append(np.s_[2 + 3 * j, 5 + j, 4:4 + s])
    v = _block_with((24, 20, 20), ch)
    return lattice_case(v, (24, 20, 20), min_points=1, max_cavities=max_cavities,
                        answer={"n_found": 6, "size": [5, 4, 3], "center": [[14.0, 9.0, 6.0], [17.0, 10.0, 5.5], [2.0, 5.0, 5.0]]})


def min_points_edge():
    """chambers of 7 and of 8 points with min_points = 8: one just under, one at the bound"""
    v = _block_with((12, 8, 12), [np.s_[2, 3, 2:9], np.s_[6, 4, 2:10]])
    return lattice_case(v, (12, 8, 12), answer={"n_found": 1, "size": [8], "center": [[6.0, 4.0, 5.5]]})


def tiny():
    """a 3 x 3 x 3 grid: the 26 outer points occupied, the middle one free and buried on all 7 lines; min_points = 1"""
    v = np.ones((3, 3, 3), bool)
    v[1, 1, 1] = False
    return lattice_case(v, (3, 3, 3), origin=(5.0, 5.0, 5.0), min_points=1,
                        answer={"n_found": 1, "size": [1], "mean_buried": [7.0], "center": [[6.0, 6.0, 6.0]]})


def empty(dims=(13, 9, 17)):
    """no atom at all (three residues, everything masked): all free, nothing buried, no cavity"""
    c = lattice_case(np.zeros((1, 1, 1), bool), dims, answer={"n_found": 0})
    c["pos"][:] = 3.0
    return c


def generic(n_res, seed):
    """a synth.make_pocket receptor with unrounded coordinates, the package's radii, water probe, default parameters, h = 1 on the
    grid that geometry.cavity_grid gives with a margin of 4 A: held to the fp32-emulating oracle, exactly"""
    import torch
    from pepflowww_amd import geometry, synth
    d = synth.make_pocket(np.random.Generator(np.random.PCG64(seed)), n_res, 1)
    pos, mask, aa = d["pos_heavyatom"][:n_res], d["mask_heavyatom"][:n_res], d["aa"][:n_res]
    origin, dims = geometry.cavity_grid(torch.from_numpy(pos)[None], torch.from_numpy(mask)[None], h=1.0, margin=4.0)
    return {"pos": pos, "mask": mask, "aa": aa, "radius": geometry.sasa_radius_table().numpy(), "origin": origin[0].numpy(),
            "dims": dims, "h": 1.0, "params": {}, "exact": False, "answer": None}


LATTICE = {"shell": shell, "shell_half": shell_half, "groove": groove, "two_equal": two_equal,
           "diagonal_6": lambda: diagonal_touch(6), "diagonal_26": lambda: diagonal_touch(26), "serpentine": serpentine,
           "many": many, "min_points_edge": min_points_edge, "tiny": tiny, "empty": empty}
GENERIC = {"generic_40": lambda: generic(40, 11), "generic_150": lambda: generic(150, 12)}
CASES = {**LATTICE, **GENERIC}
BATCH = ("shell", "groove", "empty")        # one call of B = 3: the same grid, different atom counts, one structure without atoms


def groove_receptor():
    """A receptor-sized groove for the design entry: the walls of `groove`'s box with 2 A between wall atoms (solid under the package's
    radii and a water probe), open towards +z; residues are 15 wall atoms each, type TRP.  -> (receptor dict as design.receptor_from_pdb
    gives it, apart from the torsions; (lo, hi) corners of the box's outer extent, with 4 A above its open rim: the groove lies strictly inside)."""
    import torch
    from pepflowww_amd.preprocess import residue_type
    v = box((9, 7, 11), open_top=True)
    xyz = np.argwhere(v).astype(np.float32) * 2.0
    n = (len(xyz) + 14) // 15
    xyz = np.concatenate([xyz, np.repeat(xyz[-1:], n * 15 - len(xyz), 0)])        # the last residue is filled with copies of the last atom
    pos = torch.from_numpy(xyz.reshape(n, 15, 3).copy())
    rec = {"chain_id": ["A"] * n, "chain_nb": torch.zeros(n, dtype=torch.int64), "resseq": torch.arange(1, n + 1),
           "icode": [" "] * n, "res_nb": torch.arange(1, n + 1), "aa": torch.full((n,), residue_type("TRP"), dtype=torch.int64),
           "pos_heavyatom": pos, "mask_heavyatom": torch.ones(n, 15, dtype=torch.bool)}
    return rec, (np.array([0.0, 0.0, 0.0]), np.array([16.0, 12.0, 24.0]))
